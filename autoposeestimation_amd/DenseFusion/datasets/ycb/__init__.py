"""DenseFusion/datasets/ycb: the YCB-Video data set (dataset.py) and the device builder of its samples (augment.py, csrc/ycb.hip)."""
