"""Drop-in for the reference's background_subtraction package: `segmentation_training` (reference __init__.py:25-267) trains the
7-channel background-subtraction segmentor that `utils.get_mask_prediction` labels with.  Imported lazily: the labelling half needs
neither the dataset nor the driver."""


def segmentation_training(training_config, segmentation_config, root=None, n_samples=23, **kw):
    from autoposeestimation_amd.background_subtraction.train import segmentation_training as run
    return run(training_config, segmentation_config, root=root, n_samples=n_samples, **kw)
