"""SegNet (DenseFusion/vanilla_segmentation/segnet.py) restated as one function over plain tensors, in the dtype of its input: the
yardstick of tests/test_gpu_segnet.py (float64) which tests/test_segnet_host.py first pins, bit for bit in float32, to the reference's own
class.  NCHW throughout.

Two switches take the network's branches out of the comparison with a float32 device run:
  codes   the five pools gather at the given positions (u8 [B,C,h,w], 2 * dy + dx) instead of taking their own maximum;
  masks   every ReLU is `x * mask` with the given 0 / 1 tensors instead of `max(x, 0)`."""
import torch
import torch.nn.functional as F

ENCODER = (("11", "12"), ("21", "22"), ("31", "32", "33"), ("41", "42", "43"), ("51", "52", "53"))
DECODER = (("53d", "52d", "51d"), ("43d", "42d", "41d"), ("33d", "32d", "31d"), ("22d", "21d"), ("12d", "11d"))
EPS, MOMENTUM = 1e-5, 0.1


def split_state_dict(sd, dtype):
    """state dict -> (params, bufs, nbt): parameters as leaves of `dtype`, running statistics as `dtype` clones, the step counters"""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.endswith((".weight", ".bias"))}
    bufs = {k: v.detach().to(dtype).clone() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))}
    nbt = {k: v.clone() for k, v in sd.items() if k.endswith("num_batches_tracked")}
    return params, bufs, nbt


def windows(x):
    """x[B,C,H,W] -> [B,C,H//2,W//2,4]: the 2x2 windows in scan order (0,0) (0,1) (1,0) (1,1); an odd last row / column is dropped"""
    b, c, h, w = x.shape
    ho, wo = h // 2, w // 2
    return x[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)


def own_codes(x):
    """the codes torch's CPU pool records for x[B,C,H,W]"""
    w = x.shape[3]
    _, idx = F.max_pool2d(x.detach(), 2, 2, return_indices=True)
    return (2 * ((idx // w) % 2) + (idx % w) % 2).to(torch.uint8)


def pool(x, code):
    return torch.gather(windows(x), 4, code.long().unsqueeze(-1)).squeeze(-1)


def unpool(y, code, h, w):
    b, c, ho, wo = y.shape
    win = torch.zeros(b, c, ho, wo, 4, dtype=y.dtype).scatter(4, code.long().unsqueeze(-1), y.unsqueeze(-1))
    full = win.reshape(b, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, 2 * ho, 2 * wo)
    return F.pad(full, (0, w - 2 * wo, 0, h - 2 * ho))


def forward(params, bufs, nbt, x, training, codes=None, masks=None):
    """-> (logits[B,label_nbr,H,W], info): info["relu"] the 25 ReLU outputs, info["codes"] the codes the pools used, info["own_codes"]
    the codes the pools' inputs name by themselves, info["pool_in"] those inputs.  training: batch statistics, and bufs / nbt are updated in
    place as nn.BatchNorm2d does."""
    info = {"relu": [], "codes": [], "own_codes": [], "pool_in": []}

    def layer(t, name):
        t = F.conv2d(t, params["conv%s.weight" % name], params["conv%s.bias" % name], padding=1)
        if name == "11d":
            return t
        bn = "bn%s." % name
        if training:
            nbt[bn + "num_batches_tracked"] += 1
        t = F.batch_norm(t, bufs[bn + "running_mean"], bufs[bn + "running_var"], params[bn + "weight"], params[bn + "bias"], training,
                         MOMENTUM, EPS)
        t = F.relu(t) if masks is None else t * masks[len(info["relu"])].to(t.dtype)
        info["relu"].append(t)
        return t

    sizes = []
    y = x
    for level, stage in enumerate(ENCODER):
        for name in stage:
            y = layer(y, name)
        sizes.append(tuple(y.shape[2:]))
        own = own_codes(y)
        info["pool_in"].append(y)
        info["own_codes"].append(own)
        info["codes"].append(own if codes is None else codes[level])
        y = pool(y, info["codes"][-1])
    for stage in DECODER:
        level = len(sizes) - 1
        y = unpool(y, info["codes"][level], *sizes.pop())
        for name in stage:
            y = layer(y, name)
    return y, info
