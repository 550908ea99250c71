"""DenseFusion/datasets/linemod: the LineMOD data set (dataset.py) and the device builder of its samples (augment.py, csrc/linemod.hip)."""
