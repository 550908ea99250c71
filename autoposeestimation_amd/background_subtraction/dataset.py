"""Drop-in for background_subtraction/dataset.py: `SegmentationDataset(mode, root, dirs, classes, mean=None, std=None, show_plots=False)`
over the reference's tree `<root>/<key>/{background,foreground}/img%06d.png`, `depth%06d.png`, `groundtruth/img%06d.mask.0.png`.

The reference decodes five PNGs and augments in Pillow for every sample of every epoch.  Here every file is decoded ONCE (host threads),
the raw frames stay on the device (a sample is ~3.4 MB; classes x 23 of them fit many times over), and `batch(indices)` builds a whole
batch there with two kernel launches (background_subtraction/augment.py).  `ds[i]` is a batch of one.

Random numbers are drawn on the host from the reference's generators in the reference's order (`augment.draw_params`), so seeding `random`
and `numpy.random` reproduces the reference sample for sample.  Index arithmetic as the reference (:62-64): `cls = index // n_samples`,
`key = list(classes)[cls]` -- the key comes from `classes`, not from `dirs`, so a dataset over the LAST classes (the driver's test split)
still reads the first ones; restated, not changed -- and `idx = index - cls * n_samples`.

Frames must be `size` = 480 x 640, where the reference's `transforms.Resize([480, 640])` is the identity in Pillow; any other size raises
ValueError (bilinear resizing is not restated).  `size=` is an extension for small test trees.  `mean=None` reproduces the reference's
statistics pass (:38-53), its quirks included: 23 samples per directory whatever `n_samples` is, and `x[:, :, i]` on the CHW tensor -- the
statistics of image COLUMN i over all channels and rows, not of channel i."""
import numpy as np
import torch

from autoposeestimation_amd import sharding
from autoposeestimation_amd.background_subtraction import augment as G
from autoposeestimation_amd.background_subtraction import utils as U


class Resize:
    """stands where the reference holds `transforms.Resize(size)`: the builder only provides the identity"""

    def __init__(self, size):
        self.size = tuple(size)


class SegmentationDataset:
    def __init__(self, mode, root, dirs, classes, mean=None, std=None, show_plots=False, size=(480, 640), device="cuda:0", workers=8):
        if show_plots:
            raise NotImplementedError("show_plots=True is a matplotlib debugging view of the reference; not provided")
        if not torch.cuda.is_available():
            raise RuntimeError("SegmentationDataset keeps its frames on the GPU (no CPU fallback in this build)")
        self.root, self.classes, self.dirs, self.show_plots = root, classes, dirs, show_plots
        self.n_samples = len(self.dirs[list(self.dirs.keys())[0]])
        self.n_classes = 2
        self.size = tuple(size)
        self.Resize = Resize(self.size)
        self.device = torch.device(device)
        train = mode == "train"
        self.rotation = self.hflip = self.vflip = train or None
        self.ColorJitter = G.ColorJitterPIL(brightness=0.05, contrast=0.05, saturation=0.05, hue=0.02) if train else None
        if not mean or not std:
            self.mean, self.std = self._statistics()
        else:
            self.mean, self.std = mean, std
        keys = list(self.classes)[:len(self.dirs)]
        items = [(k, i) for k in keys for i in range(self.n_samples)]
        frames = list(sharding.prefetched(items, lambda it: self._read(*it), workers=workers))
        # one resident tensor per kind; a sample is five views into them
        self._res = [torch.from_numpy(np.stack([f[j] for f in frames])).to(self.device) for j in range(5)] if frames else None

    def _read(self, key, idx):
        frames = U.read_sample(self.root, key, idx)
        if frames[4].shape != self.size:
            raise ValueError("frame %s/%d is %d x %d, not %d x %d: the reference resizes every frame to [480, 640] bilinearly, which is only "
                             "the identity for frames of that size; other sizes are not provided" % ((key, idx) + frames[4].shape + self.size))
        return frames

    def _statistics(self):
        print("__________________________________________________")
        print("getting mean and std")
        means, stds = [], []
        for key in self.dirs:
            for idx in range(23):
                x, _ = U.load_subtraction(self.root, key, idx)
                n = x.shape[2]
                x = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).float().div(255)        # ToTensor
                means.append([torch.mean(x[:, :, i]).numpy() for i in range(n)])
                stds.append([torch.std(x[:, :, i]).numpy() for i in range(n)])
        mean, std = list(np.mean(np.array(means), axis=0)), list(np.mean(np.array(stds), axis=0))
        print("mean: {}\n std: {}".format(mean, std))
        return mean, std

    def draw(self):
        """the augmentation of one sample, drawn as the reference draws it"""
        return G.draw_params(rotate=self.rotation, hflip=self.hflip, vflip=self.vflip, jitter=self.ColorJitter)

    def batch(self, indices, params=None, want_u8=False):
        """-> x[B,7,H,W] f32 (a channels-last view of the builder's x8[B,H,W,8]), y[B,H,W] i64; draws one parameter set per sample, in
        index order, unless `params` gives them"""
        indices = [int(i) for i in indices]
        for i in indices:
            if not 0 <= i < len(self):
                raise IndexError("index %d outside the %d samples" % (i, len(self)))
        if params is None:
            params = [self.draw() for _ in indices]
        samples = [tuple(r[i] for r in self._res) for i in indices]
        out = G.build_samples(samples, params, self.mean, self.std, want_u8=want_u8)
        x = out[0].permute(0, 3, 1, 2)[:, :7]
        return (x, out[1], out[2]) if want_u8 else (x, out[1])

    def __getitem__(self, index):
        cls = index // self.n_samples
        idx = int(index - (cls * self.n_samples))
        x, y = self.batch([cls * self.n_samples + idx])
        return x[0], y[0]

    def __len__(self):
        return int(self.n_samples * len(self.dirs.keys()))
