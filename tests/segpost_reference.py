"""Plain restatement of the segmentation post-processing path (csrc/segpost.hip, ccl.h, seg_head.h): numpy and Python integers, no device
code, no scipy.  tests/test_segpost_host.py checks it against oracle/densefusion_oracle.py and scipy where both are defined;
tests/test_gpu_segpost_edges.py compares the kernels with it on the inputs of tests/segpost_edge_cases.py.

Every rule stands in one place and has a switch in `rules`, so that the host test can show which cases a wrong rule fails:
    connectivity   8 | 4
    threshold      "gt" (count > min_pixels) | "ge"
    count          "class" (pixels of the class in the frame) | "component"
    ties           "first" (strict >, raster order) | "last"
    depth          "ne0" (depth != 0 on the unsigned value) | "signed_gt0" (int16 view > 0)
    wrap           "start" (np.pad wrap: cand[i % n]) | "end"
    offset         "u" (floor((i + u) n / N)) | "none"
A mode of SUM with the rule "mean_for_sum" scores by the mean instead."""
import numpy as np

from oracle import densefusion_oracle as O

MEAN, SUM = 0, 1
RULES = dict(connectivity=8, threshold="gt", count="class", ties="first", depth="ne0", wrap="start", offset="u", score="as_mode")
_N8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
_N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
_M32 = 0xFFFFFFFF


def _rules(rules):
    r = dict(RULES)
    r.update(rules or {})
    return r


def flood(lab, C, connectivity=8):
    """lab[H,W] -> id[H,W] int64: the smallest raster index of the pixel's component (same class in [1, C), 8-connectivity), -1 elsewhere"""
    H, W = lab.shape
    nb = _N8 if connectivity == 8 else _N4
    lab_l = np.where(lab < C, lab, 0).astype(np.int64).ravel().tolist()
    ids = [-1] * (H * W)
    for root in np.nonzero(lab_l)[0].tolist():              # raster order: the first unvisited pixel of a component is its smallest index
        if ids[root] >= 0:
            continue
        c = lab_l[root]
        ids[root] = root
        stack = [root]
        while stack:
            p = stack.pop()
            y, x = divmod(p, W)
            for dy, dx in nb:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W:
                    q = v * W + u
                    if lab_l[q] == c and ids[q] < 0:
                        ids[q] = root
                        stack.append(q)
    return np.array(ids, np.int64).reshape(H, W)


def exact_int(score):
    """float32 array -> Python ints: the exact value times 2^149 (every float32 is a multiple of 2^-149)"""
    return [int(v) for v in (np.asarray(score, np.float32).astype(np.float64) * 2.0 ** 149).ravel()]


def components_frame(lab, score, C, min_pixels, mode, rules=None):
    """-> objmap[H,W] u8, tight {cls: (rmin, rmax, cmin, cmax) inclusive}, best {cls: (root, (sum * 2^149, count), second)}: per class the
    winning component and the runner-up's score (None when the class has one component)"""
    r = _rules(rules)
    H, W = lab.shape
    ids = flood(lab, C, r["connectivity"])
    objmap = np.zeros((H, W), np.uint8)
    tight, best = {}, {}
    sc = exact_int(score)
    flat_ids, flat_lab = ids.ravel(), lab.ravel()
    use_mean = mode == MEAN or r["score"] == "mean_for_sum"
    for c in range(1, C):
        idx = np.nonzero(flat_lab == c)[0]
        if len(idx) == 0:
            continue
        comps = {}
        for p, root in zip(idx.tolist(), flat_ids[idx].tolist()):
            s = comps.setdefault(root, [0, 0])
            s[0] += sc[p]
            s[1] += 1
        win, win_s, scores = None, (0, 1), []
        for root in sorted(comps):
            s, n = comps[root]
            counted = len(idx) if r["count"] == "class" else n
            if not (counted > min_pixels if r["threshold"] == "gt" else counted >= min_pixels):
                continue
            val = (s, n) if use_mean else (s, 1)
            scores.append(val)
            bigger = val[0] * win_s[1] > win_s[0] * val[1]
            equal = val[0] * win_s[1] == win_s[0] * val[1]
            if win is None or bigger or (equal and r["ties"] == "last"):     # biggest = 1 by default, then strict '>'
                win, win_s = root, val
        if win is None:
            continue
        m = ids == win
        objmap[m] = c
        rr, cc = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        tight[c] = (int(rr[0]), int(rr[-1]), int(cc[0]), int(cc[-1]))
        rest = sorted(scores, key=lambda v: -v[0] / v[1])
        best[c] = (win, win_s, rest[1] if len(rest) > 1 else None)
    return objmap, tight, best


def components(label, score, C, min_pixels, mode, rules=None):
    """label[B,H,W] u8, score[B,H,W] f32 -> objmap[B,H,W] u8, tight[B,C,4] (inclusive extents, -1 where none), det[B,C,5], best (per frame)"""
    B, H, W = label.shape
    objmap = np.zeros((B, H, W), np.uint8)
    tight = np.full((B, C, 4), -1, np.int64)
    det = np.zeros((B, C, 5), np.int32)
    best = []
    for b in range(B):
        om, t, bst = components_frame(label[b], score[b], C, min_pixels, mode, rules)
        objmap[b] = om
        best.append(bst)
        for c, ext in t.items():
            tight[b, c] = ext
            det[b, c] = (1,) + tuple(O.get_bbox(om == c, H, W))
    return objmap, tight, det, best


def hash32(seed, o):
    h = (seed ^ ((0x9E3779B9 * (o + 1)) & _M32)) & _M32
    h ^= h >> 16
    h = (h * 0x7feb352d) & _M32
    h ^= h >> 15
    h = (h * 0x846ca68b) & _M32
    h ^= h >> 16
    return h


def candidates(objmap, depth, obj, rules=None):
    r = _rules(rules)
    b, cls, rmin, rmax, cmin, cmax = [int(v) for v in obj]
    d = depth[b, rmin:rmax, cmin:cmax]
    has = d != 0 if r["depth"] == "ne0" else d.view(np.int16) > 0
    return np.nonzero(((objmap[b, rmin:rmax, cmin:cmax] == cls) & has).ravel())[0].astype(np.int64)


def pick(n, N, seed, o, rules=None):
    """positions in the candidate list, n > N: j_i = min(n - 1, floor((i + u) n / N)), one IEEE double operation each"""
    r = _rules(rules)
    u = np.float64(hash32(seed, o)) / np.float64(4294967296.0) if r["offset"] == "u" else np.float64(0.0)
    i = np.arange(N, dtype=np.float64)
    j = np.floor(((i + u) * np.float64(n)) / np.float64(N)).astype(np.int64)
    return np.minimum(j, n - 1)


def choose(objmap, depth, objects, N, seed, rules=None):
    """-> choose[n,N] i64 (zeros for an object without candidates), n_cand[n] i32"""
    r = _rules(rules)
    objects = np.asarray(objects).reshape(-1, 6)
    out = np.zeros((len(objects), N), np.int64)
    n_cand = np.zeros(len(objects), np.int32)
    for o, obj in enumerate(objects):
        cand = candidates(objmap, depth, obj, rules)
        n = len(cand)
        n_cand[o] = n
        if n == 0:
            continue
        if n > N:
            j = pick(n, N, seed, o, rules)
            assert np.all(np.diff(j) > 0) and j[-1] < n          # the properties on their own: strictly increasing, all < n
            out[o] = cand[j]
        elif r["wrap"] == "start":
            out[o] = cand[np.arange(N) % n]                       # np.pad(cand, (0, N - n), "wrap")
        else:
            out[o] = np.concatenate([cand, cand[::-1][np.arange(N - n) % n]]) if N > n else cand
    return out, n_cand


def backproject(depth_frame, ch, rmin, rmax, cmin, cmax, intr, depth_scale):
    return O.backproject(depth_frame, ch, rmin, rmax, cmin, cmax, {"intr": intr, "depth_scale": depth_scale})


def _softmax64(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def argmax_score(logits, C, double):
    """logits[npix, >= C] (float32, or float64 from `head`) -> label[npix] u8, score[npix] f64, unsure[npix] bool.
    score: the top probability after one or two softmaxes in float64.  label: the lowest class whose float32 torch-CPU final probability
    equals the maximum's (the reference's torch.argmax of what it holds).  unsure: the top two float64 final probabilities lie within 1e-6
    (relative) of each other -- the pixels a label comparison may leave out."""
    import torch
    import torch.nn.functional as F
    l64 = np.asarray(logits)[:, :C].astype(np.float64)
    p = _softmax64(l64)
    if double:
        p = _softmax64(p)
    score = p.max(-1)
    if C > 1:
        top = np.partition(p, C - 2, axis=-1)[:, C - 2:]
        unsure = (top[:, 1] - top[:, 0]) <= 1e-6 * top[:, 1]
    else:
        unsure = np.zeros(len(p), bool)
    t = torch.from_numpy(np.ascontiguousarray(l64.astype(np.float32)))
    q = F.softmax(t, -1)
    if double:
        q = F.softmax(q, -1)
    q = q.numpy()
    label = (q == q.max(-1, keepdims=True)).argmax(-1).astype(np.uint8)
    return label, score, unsure


def head(feat, w, bias, C, double):
    """feat[npix,64] f32, w[C,64] f32, bias[C] f32 or None: the float64 contraction, then argmax_score"""
    logits = feat.astype(np.float64) @ w[:C].astype(np.float64).T
    if bias is not None:
        logits = logits + bias[:C].astype(np.float64)
    return argmax_score(logits, C, double)


def trust_counts(objmap, cls, bs_label, depth, gate, cut0, cut1):
    """label_generator/create_labels.py:166-196 with the depth gate of :111-112 -> counts[B,6] =
    (bs & pred, bs & !pred, depth & pred, depth & !pred, centre & pred, centre & !pred)"""
    B, H, W = objmap.shape
    out = np.zeros((B, 6), np.uint32)
    for b in range(B):
        pred = objmap[b] == cls
        d = depth[b].astype(np.float64)
        d[d > np.float64(gate[b, 1])] = 0                       # depth[depth > max_measure_dist] = 0
        d[d < np.float64(gate[b, 0])] = 0                       # depth[depth < min_measure_dist] = 0
        win = np.zeros((H, W), bool)
        win[cut0:max(H - cut0, 0), cut1:max(W - cut1, 0)] = True
        conds = (bs_label[b] != 0 if bs_label is not None else np.zeros((H, W), bool), d != 0, win)
        for k, cond in enumerate(conds):
            out[b, 2 * k] = np.count_nonzero(cond & pred)
            out[b, 2 * k + 1] = np.count_nonzero(cond & ~pred)
    return out


def preprocess(rgb, rects, hc, wc, div255):
    """rgb[B,H,W,3] u8, rects[n,3] (frame,row0,col0) -> [n,hc,wc,4] f32: torch CPU float32 (x[/255] - mean) / std, channel 3 = 0"""
    import torch
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
    out = torch.zeros(len(rects), hc, wc, 4, dtype=torch.float32)
    for i, (b, r0, c0) in enumerate(np.asarray(rects).reshape(-1, 3).tolist()):
        x = torch.from_numpy(np.ascontiguousarray(rgb[b, r0:r0 + hc, c0:c0 + wc])).float()
        if div255:
            x = x.div(255)
        out[i, :, :, :3] = (x - mean) / std
    return out.numpy()
