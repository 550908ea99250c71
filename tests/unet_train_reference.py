"""fp64 train-mode restatement of smp 0.1.3's Unet (resnet18 / resnet34 encoder) for tests/test_gpu_seg_train.py, written with
torch.nn.functional only: every BatchNorm2d is F.batch_norm(training=True, momentum=0.1, eps=1e-5) on the batch's statistics, updating
copies of the running buffers.  `params` maps smp's state-dict keys to fp64 tensors (leaves, so torch autograd gives the reference
gradients); `buffers` holds the running_mean / running_var copies the call updates in place."""
import torch
import torch.nn.functional as F

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def split_state(sd, device="cpu"):
    """state dict -> (params fp64 leaves requiring grad, running buffers fp64, num_batches_tracked ints)"""
    params, bufs, nbt = {}, {}, {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            nbt[k] = int(v)
        elif k.endswith("running_mean") or k.endswith("running_var"):
            bufs[k] = v.detach().to(device, torch.float64).clone()
        else:
            params[k] = v.detach().to(device, torch.float64).clone().requires_grad_(True)
    return params, bufs, nbt


def _bn(x, p, bufs, nbt, prefix, training):
    if training:
        nbt[prefix + ".num_batches_tracked"] = nbt.get(prefix + ".num_batches_tracked", 0) + 1
    return F.batch_norm(x, bufs[prefix + ".running_mean"], bufs[prefix + ".running_var"], p[prefix + ".weight"], p[prefix + ".bias"],
                        training=training, momentum=0.1, eps=1e-5)


def forward(p, bufs, nbt, x, encoder="resnet34", activation="softmax", training=True, margins=None):
    """x[B,in,H,W] fp64 -> the model output [B,classes,H,W] (activation applied), NCHW.  margins: a list that receives, per ReLU, the
    smallest |pre-activation| (how close an fp32 evaluation may come to flipping a ReLU mask)"""
    bn = lambda t, k: _bn(t, p, bufs, nbt, k, training)  # noqa: E731
    if margins is not None:
        def relu(t):
            margins.append(float(t.detach().abs().min()))
            return F.relu(t)
    else:
        relu = F.relu
    y = relu(bn(F.conv2d(x, p["encoder.conv1.weight"], stride=2, padding=3), "encoder.bn1"))
    feats = [y]
    y = F.max_pool2d(y, 3, 2, 1)
    for li, n in enumerate(BLOCKS[encoder], 1):
        for b in range(n):
            k = "encoder.layer%d.%d." % (li, b)
            s = 2 if (b == 0 and li > 1) else 1
            if k + "downsample.0.weight" in p:
                res = bn(F.conv2d(y, p[k + "downsample.0.weight"], stride=s), k + "downsample.1")
            else:
                res = y
            t = relu(bn(F.conv2d(y, p[k + "conv1.weight"], stride=s, padding=1), k + "bn1"))
            y = relu(bn(F.conv2d(t, p[k + "conv2.weight"], padding=1), k + "bn2") + res)
        feats.append(y)
    y = feats[4]
    for i, skip in enumerate((feats[3], feats[2], feats[1], feats[0], None)):
        k = "decoder.blocks.%d." % i
        y = F.interpolate(y, scale_factor=2, mode="nearest")
        if skip is not None:
            y = torch.cat([y, skip], 1)
        y = relu(bn(F.conv2d(y, p[k + "conv1.0.weight"], padding=1), k + "conv1.1"))
        y = relu(bn(F.conv2d(y, p[k + "conv2.0.weight"], padding=1), k + "conv2.1"))
    y = F.conv2d(y, p["segmentation_head.0.weight"], p["segmentation_head.0.bias"], padding=1)
    return torch.softmax(y, 1) if activation in ("softmax", "softmax2d") else y
