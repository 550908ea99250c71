"""DenseFusion/vanilla_segmentation on gfx950: the SegNet that produces the `segnet_results` label maps the LineMOD evaluation reads,
its cross-entropy loss, the YCB-Video sample source and the training / labelling drivers."""
