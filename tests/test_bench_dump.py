"""bench.py --dump-outputs on the host side: the types it writes, the 64 MB limit and the fixed sample of an output larger than its share
(the GPU run itself: tests/test_gpu_bench_cli.py)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_types_limit_and_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"poses": torch.randn(64, 1, 8, generator=g), "pose": torch.randn(64, 7, generator=g, dtype=torch.float64),
              "objects": [(k, 1, 2, 3, 4, 5) for k in range(64)], "choose": torch.randint(0, 307200, (64, 1000), generator=g),
              "wide": torch.tensor([2 ** 40 + 1, 3]), "objmap": torch.randint(0, 13, (64, 480, 640), generator=g, dtype=torch.uint8)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == set(arrays)
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in a) <= 64 << 20
    assert a["poses"].dtype == np.float32 and np.array_equal(a["poses"], arrays["poses"].numpy())
    assert a["pose"].dtype == np.float64 and np.array_equal(a["pose"], arrays["pose"].numpy())
    assert a["objects"].dtype == np.float32 and np.array_equal(a["objects"], np.asarray(arrays["objects"]))
    assert a["choose"].dtype == np.float32 and np.array_equal(a["choose"], arrays["choose"].numpy())
    assert a["wide"].dtype == np.float64 and a["wide"][0] == 2 ** 40 + 1          # beyond float32's exact integers
    # the 78 MB object map (as float32) is sampled: the same positions in every run
    om = a["objmap"]
    assert om.dtype == np.float32 and om.ndim == 1 and 0 < om.size < arrays["objmap"].numel()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert set(np.unique(om)) <= set(range(13))
