"""fp64 numpy restatement of the VQ-NNF template matcher's arithmetic (test infrastructure).

Restates marie/components/template_matching/vqnnf/matching/{feature_extraction,kmeans,template_matching,gauss_haar_filters}.py
and the peak / box arithmetic of vqnnf_template_matching.py:184-202,307 in float64, with the tie rules the fp32 reference
follows (first maximum).  tests/test_vqnnf_cpu.py pins it to tests/golden/vqnnf.npz (written by the reference's own code);
the GPU tests compare the HIP kernels against it.
"""
from __future__ import annotations

import json
import os

import numpy as np

# torch.roll shifts over (rows, cols), in the order of feature_extraction.py:53-66
SHIFTS = ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))
SUPPRESSED = -0.82
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vqnnf.npz")


def load_golden():
    """-> (arrays by "<case>/<name>", metadata) of tests/golden/vqnnf.npz (tools/gen_vqnnf_golden.py)"""
    z = np.load(GOLDEN)
    arrays = {k: z[k] for k in z.files if k != "meta"}
    return arrays, json.loads(bytes(z["meta"]).decode())


def clip_pairs(window: np.ndarray):
    """the four 224 x 224 x 3 clip pairs of the cosine checks, built from a golden window: identical, shifted by one
    pixel, inverted, all-white against all-white"""
    base = np.tile(window, (3, 2, 1))[:224, :224].copy()
    white = np.full_like(base, 255)
    return [(base, base.copy()), (base, np.roll(base, 1, axis=1)), (base, 255 - base), (white, white.copy())]


def color_features(img: np.ndarray) -> np.ndarray:
    """HxWx3 uint8 -> (27, H, W) float64: every pixel's RGB and its eight neighbours (wrapping around the image's own
    edges), / 255.  The values are the fp32 quotients the reference forms, held in float64."""
    x = (np.asarray(img, np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255)).astype(np.float64)
    return np.concatenate([np.roll(x, s, axis=(1, 2)) for s in SHIFTS], axis=0)


def rect_features(img: np.ndarray, rect) -> np.ndarray:
    """features of the pixels of rect (x, y, w, h) of img, row-major: (h*w, 27)"""
    x, y, w, h = (int(v) for v in rect)
    f = color_features(img)[:, y:y + h, x:x + w]
    return f.reshape(27, -1).T.copy()


def sq_distances(feats: np.ndarray, codebook: np.ndarray) -> np.ndarray:
    """(n, 27), (K, 27) -> squared Euclidean distances (n, K): the squared differences added one by one in feature order,
    each product and each sum rounded to float64 — the order and the roundings of csrc/vqnnf.hip's vq_nearest, so the two
    agree bit for bit, ties included."""
    feats, codebook = np.asarray(feats, np.float64), np.asarray(codebook, np.float64)
    out = np.zeros((feats.shape[0], codebook.shape[0]))
    for j in range(feats.shape[1]):
        e = feats[:, j][:, None] - codebook[:, j][None, :]
        out = out + e * e
    return out


def distances(feats: np.ndarray, codebook: np.ndarray) -> np.ndarray:
    """Euclidean distances (n, K)"""
    return np.sqrt(sq_distances(feats, codebook))


def assign(feats: np.ndarray, codebook: np.ndarray):
    """nearest code per row, equal distances to the lowest index -> (codes int64 (n,), gap (n,)): gap is the Euclidean
    distance from the best to the second-best *distinct* distance (inf when every code is equally far)."""
    d2 = sq_distances(feats, codebook)
    codes = d2.argmin(axis=1)
    best = d2[np.arange(d2.shape[0]), codes]
    rest = np.where(d2 > best[:, None], d2, np.inf)
    return codes, np.sqrt(rest.min(axis=1)) - np.sqrt(best)


def codes_match(got: np.ndarray, want: np.ndarray, gap: np.ndarray, eps: float):
    """the rule of the assignment checks: a pixel may differ only where gap < eps -> (ok, fraction set aside)"""
    got, want = np.asarray(got).reshape(-1).astype(np.int64), np.asarray(want).reshape(-1).astype(np.int64)
    differs = got != want
    return bool(np.all(gap.reshape(-1)[differs] < eps)), float(differs.mean())


def kmeans_step(feats: np.ndarray, centroids: np.ndarray):
    """one iteration of KMeans.fit_predict (kmeans.py:219-238, minibatch=None) -> (labels, new centroids, error, gap)"""
    centroids = np.asarray(centroids, np.float64)
    labels, gap = assign(feats, centroids)
    new = np.zeros_like(centroids)
    for k in range(centroids.shape[0]):
        m = labels == k
        if m.any():
            new[k] = feats[m].mean(axis=0)
    return labels, new, float(((new - centroids) ** 2).sum()), gap


def kmeans_fit(feats: np.ndarray, init_idx, max_iter: int = 25, tol: float = 1e-4):
    """-> (labels of the last assignment, codebook, iterations run, centroids after every iteration)"""
    cent = feats[np.asarray(init_idx, np.int64)].copy()
    trail, labels = [], None
    for it in range(max_iter):
        labels, cent, err, _ = kmeans_step(feats, cent)
        trail.append(cent)
        if err <= tol:
            break
    return labels, cent, it + 1, trail


def n_code_of(w: int, h: int, n_code: int = 128) -> int:
    return n_code if w * h > n_code else w * h


# ------------------------------------------------------------------------------------------------ Gauss-Haar filters
def gauss_box_3x3(sigma: float = 2.0) -> np.ndarray:
    """get_gaussian_box_filter((3, 3), sigma): a centred unit impulse through scipy.ndimage.gaussian_filter (mode
    'reflect', truncate 4.0), rounded to fp32 as the reference's tensor is."""
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    wts = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    wts /= wts.sum()
    line = np.pad(np.array([0.0, 1.0, 0.0]), radius, mode="symmetric")
    g = np.array([np.dot(wts, line[i:i + 2 * radius + 1]) for i in range(3)])
    return np.outer(g, g).astype(np.float32)


def integral_taps(box: np.ndarray) -> np.ndarray:
    """convert_box_to_integral (utils.py:12-18) in fp32, then / 16 (gauss_haar_filters.py:205-207) -> 4x4 fp32"""
    mult = np.array([[1, -1], [-1, 1]], np.float32)
    out = np.zeros((box.shape[0] + 1, box.shape[1] + 1), np.float32)
    for i in range(box.shape[0]):
        for j in range(box.shape[1]):
            out[i:i + 2, j:j + 2] += np.float32(box[i, j]) * mult
    return out / np.float32(out.shape[0] * out.shape[1])


def filter_bank(t_rows: int, t_cols: int, n_scales: int = 3):
    """GaussHaarFilters(filters=1, n_scales=3, kernel_size=3, sigma=2) for a template of t_rows x t_cols: haar_1x is listed
    twice, so 2 * n_scales filters -> (taps (F,4,4) fp32, dilation (F,2) int, kernel (F,2) int, weight (F,) float64)."""
    taps1 = integral_taps(gauss_box_3x3(2.0))
    taps, dil, ker, wgt = [], [], [], []
    for scale in np.linspace(1, 1 / n_scales, n_scales):
        w, h = int(t_rows * scale), int(t_cols * scale)
        for _ in range(2):
            d = (w // 3, h // 3)
            taps.append(taps1)
            dil.append(d)
            ker.append((3 * d[0] + 1, 3 * d[1] + 1))
            wgt.append(float(scale) * 1.0)
    return np.stack(taps), np.asarray(dil, np.int64), np.asarray(ker, np.int64), np.asarray(wgt, np.float64)


def integral_of(codes: np.ndarray, K: int) -> np.ndarray:
    """(H, W) codes -> (K, H, W) float64 double cumulative sum of the one-hot, no leading zero row / column"""
    onehot = (np.asarray(codes)[None, :, :] == np.arange(K)[:, None, None]).astype(np.float64)
    return onehot.cumsum(axis=1).cumsum(axis=2)


def _responses(integral: np.ndarray, taps: np.ndarray, dil) -> np.ndarray:
    """valid dilated 4x4 correlation per channel: (K, H, W) -> (K, H - 3 dx, W - 3 dy)"""
    K, H, W = integral.shape
    dx, dy = int(dil[0]), int(dil[1])
    hv, wv = H - 3 * dx, W - 3 * dy
    y = np.zeros((K, hv, wv))
    for a in range(4):
        for b in range(4):
            y += float(taps[a, b]) * integral[:, a * dx:a * dx + hv, b * dy:b * dy + wv]
    return y


def template_responses(labels: np.ndarray, K: int, taps, dil, ker) -> np.ndarray:
    """get_template_features: (t_rows, t_cols) labels -> (F, K): reflect padding of the integral image when a kernel
    exceeds the template, then the (1, 1) centre crop of the valid responses."""
    integral = integral_of(labels, K)
    out = np.zeros((len(taps), K))
    for f in range(len(taps)):
        px = max(0, int(np.ceil((ker[f][0] - integral.shape[1]) / 2)))
        py = max(0, int(np.ceil((ker[f][1] - integral.shape[2]) / 2)))
        y = _responses(np.pad(integral, ((0, 0), (px, px), (py, py)), mode="reflect"), taps[f], dil[f])
        x1 = (y.shape[1] - 1) // 2 if y.shape[1] > 1 else 0
        y1 = (y.shape[2] - 1) // 2 if y.shape[2] > 1 else 0
        out[f] = y[:, x1, y1]
    return out


def heatmap(codes: np.ndarray, K: int, tmpl: np.ndarray, taps, dil, wgt):
    """get_query_map -> (heat (H, W), per-filter minima (F,))"""
    H, W = codes.shape
    integral = integral_of(codes, K)
    heat = np.zeros((H, W))
    mins = np.zeros(len(taps))
    for f in range(len(taps)):
        y = _responses(integral, taps[f], dil[f])
        sim = -(np.abs(y - np.asarray(tmpl[f], np.float64)[:, None, None]) * (1.0 / K)).sum(axis=0) * float(wgt[f])
        mins[f] = sim.min()
        full = np.full((H, W), mins[f])
        top, left = (H - sim.shape[0]) // 2, (W - sim.shape[1]) // 2
        full[top:top + sim.shape[0], left:left + sim.shape[1]] = sim
        heat += full
    return heat, mins


# ------------------------------------------------------------------------------------------------ peaks and boxes
def odd(f) -> int:
    return int(np.ceil(f)) // 2 * 2 + 1


def peaks(heat: np.ndarray, box_w: int, box_h: int, max_objects: int):
    """vqnnf_template_matching.py:184-202,307 on a copy of heat -> [(row, col, value, (x, y, w, h))]"""
    heat = np.array(heat, copy=True)
    out = []
    query_w, query_h = box_h, box_w            # swapped, as there
    for _ in range(max_objects):
        r, c = np.unravel_index(np.argmax(heat), heat.shape)
        val = heat[r, c]
        qx = int(r + 1 - (odd(query_w) - 1) / 2)
        qy = int(c + 1 - (odd(query_h) - 1) / 2)
        out.append((int(r), int(c), float(val), (qy, qx, query_h, query_w)))
        heat[qx:qx + query_w, qy:qy + query_h] = SUPPRESSED
    return out


def clip_cosine(a: np.ndarray, b: np.ndarray, eps: float = 1e-8) -> float:
    """nn.CosineSimilarity(dim=1) of the flattened colour features of two HxWx3 uint8 clips"""
    fa, fb = color_features(a).reshape(-1), color_features(b).reshape(-1)
    return float(np.dot(fa, fb) / (max(np.sqrt(np.dot(fa, fa)), eps) * max(np.sqrt(np.dot(fb, fb)), eps)))
