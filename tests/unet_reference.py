"""CPU restatement of smp 0.1.3's Unet forward (segmentation/unet.py's docstring) straight from a state dict, with torch.nn.functional
and the BatchNorm layers left unfolded (eval mode, running statistics).  Test infrastructure: fp64 for the small cases."""
import torch
import torch.nn.functional as F

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def encoder(sd, x, name="resnet34"):
    """x[B,C,H,W] -> [f1..f5]"""
    f1 = F.relu(_bn(sd, "encoder.bn1", F.conv2d(x, sd["encoder.conv1.weight"], None, 2, 3)))
    y = F.max_pool2d(f1, 3, 2, 1)
    feats = [f1]
    for li, n in enumerate(BLOCKS[name], 1):
        for b in range(n):
            p = "encoder.layer%d.%d." % (li, b)
            s = 2 if (b == 0 and li > 1) else 1
            t = F.relu(_bn(sd, p + "bn1", F.conv2d(y, sd[p + "conv1.weight"], None, s, 1)))
            t = _bn(sd, p + "bn2", F.conv2d(t, sd[p + "conv2.weight"], None, 1, 1))
            res = y if (p + "downsample.0.weight") not in sd else _bn(sd, p + "downsample.1", F.conv2d(y, sd[p + "downsample.0.weight"], None, s))
            y = F.relu(t + res)
        feats.append(y)
    return feats


def decoder_block(sd, i, x, skip):
    p = "decoder.blocks.%d." % i
    x = F.interpolate(x, scale_factor=2, mode="nearest")
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    x = F.relu(_bn(sd, p + "conv1.1", F.conv2d(x, sd[p + "conv1.0.weight"], None, 1, 1)))
    return F.relu(_bn(sd, p + "conv2.1", F.conv2d(x, sd[p + "conv2.0.weight"], None, 1, 1)))


def features(sd, x, name="resnet34"):
    f = encoder(sd, x, name)
    y = f[4]
    for i, skip in enumerate((f[3], f[2], f[1], f[0], None)):
        y = decoder_block(sd, i, y, skip)
    return y


def logits(sd, x, name="resnet34", dtype=torch.float64):
    """x[B,C,H,W] -> raw head logits [B,classes,H,W] (before the activation), computed in `dtype`"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    f = features(sd, x.to(dtype), name)
    return F.conv2d(f, sd["segmentation_head.0.weight"], sd["segmentation_head.0.bias"], 1, 1)
