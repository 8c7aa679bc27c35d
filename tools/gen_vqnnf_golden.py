"""Writes tests/golden/vqnnf.npz: small inputs and the results the reference's own VQ-NNF code computes on them.

    python tools/gen_vqnnf_golden.py --reference /path/to/marie-ai

The five files of marie/components/template_matching/vqnnf/matching/ that hold the matching core ({template_matching,kmeans,
init_methods,gauss_haar_filters,utils}.py) are pure torch.  They are loaded by path under empty stand-ins for the modules
they import and never call with verbose=False (cv2, colorcet, seaborn, skimage.color, skimage.exposure);
KMeans.remaining_memory, which asks torch.cuda for the memory of a CPU device, is replaced by a constant.

Per case (a window, a template frame and box) the file records the window, the frame, the box, the initial centroid indices,
the centroids after iterations 1, 2, last - 1 and last, the stop iteration, the returned labels, the 6 x K template
responses, the filter descriptors, the query code map, the heat map and the max_objects = 2 peaks and boxes.  It also
records how far the reference's fp32 results are from an fp64 evaluation — the bars of tests/test_vqnnf_gpu.py are 4x those —
and asserts the conditions under which the tests set nothing aside (see the asserts below).
"""
from __future__ import annotations

import argparse
import copy
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vqnnf_ref as R  # noqa: E402

TOL = 1e-4
MAX_ITER = 25


def load_reference(ref_root: str):
    for name in ("cv2", "colorcet", "seaborn", "skimage", "skimage.color", "skimage.exposure"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.color"].label2rgb = None
    sys.modules["skimage.exposure"].rescale_intensity = None
    pkg = types.ModuleType("_vqnnf_matching")
    pkg.__path__ = [os.path.join(ref_root, "marie", "components", "template_matching", "vqnnf", "matching")]
    sys.modules["_vqnnf_matching"] = pkg
    tm = importlib.import_module("_vqnnf_matching.template_matching")
    km = importlib.import_module("_vqnnf_matching.kmeans")
    km.KMeans.remaining_memory = lambda self, device=None: 1 << 30
    return tm, km


# ------------------------------------------------------------------------------------------------------- synthetic pages
def textured(rng, h, w, blobs):
    """seeded blobs on white plus a smooth gradient region (white gives the duplicate centroids, the rest distinct ones)"""
    img = np.full((h, w, 3), 255, np.uint8)
    gy, gx = h // 3, w // 3
    yy, xx = np.mgrid[0:gy, 0:gx]
    img[h - gy:, :gx, 0] = (40 + 200 * xx / max(gx - 1, 1)).astype(np.uint8)
    img[h - gy:, :gx, 1] = (230 - 180 * yy / max(gy - 1, 1)).astype(np.uint8)
    img[h - gy:, :gx, 2] = ((xx + yy) * 255 // (gx + gy)).astype(np.uint8)
    for _ in range(blobs):
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        ry, rx = rng.integers(1, 5), rng.integers(1, 7)
        col = rng.integers(0, 200, 3)
        y0, y1, x0, x1 = max(0, cy - ry), min(h, cy + ry + 1), max(0, cx - rx), min(w, cx + rx + 1)
        sy, sx = np.mgrid[y0:y1, x0:x1]
        m = ((sy - cy) / (ry + 0.5)) ** 2 + ((sx - cx) / (rx + 0.5)) ** 2 <= 1
        # every blob pixel a little off the blob's colour: flat blobs give mirrored centroids (a blob's left and right edge)
        # that tie exactly for every pixel between them, and fp32 rounding then decides the reference's k-means labels
        noisy = np.clip(col[None, None, :] + rng.integers(-12, 13, (y1 - y0, x1 - x0, 3)), 0, 255).astype(np.uint8)
        img[y0:y1, x0:x1][m] = noisy[m]
    return img


def make_case(seed, win_hw, box_hw, frame_xy, plant_xy):
    """the template frame (box at frame_xy), and a window of other texture with the template's pixels planted at plant_xy"""
    rng = np.random.default_rng(seed)
    H, W = win_hw
    bh, bw = box_hw
    frame = textured(rng, H, W, H * W // 60)
    window = textured(rng, H, W, H * W // 60)
    fx, fy = frame_xy
    px, py = plant_xy
    window[py:py + bh, px:px + bw] = frame[fy:fy + bh, fx:fx + bw]
    return window, frame, (fx, fy, bw, bh)


CASES = (  # name, seed, window (H, W), template (rows, cols), box origin in the frame (x, y), planted at (x, y)
    ("a36x20", 11, (96, 128), (36, 20), (50, 20), (30, 40)),
    ("a9x11", 12, (96, 128), (9, 11), (20, 60), (90, 25)),
    ("a21x33", 13, (96, 128), (21, 33), (60, 40), (2, 1)),       # peak within half a kernel of the border
    ("b36x20", 14, (61, 83), (36, 20), (10, 12), (52, 20)),
    ("b9x11", 15, (61, 83), (9, 11), (8, 44), (60, 7)),        # the box lies in the gradient region
    ("b21x33", 16, (61, 83), (21, 33), (30, 5), (48, 38)),       # near the right / bottom border
)


def feats_of(img):
    """the reference's colour features (feature_extraction.py:48-67; that file imports albumentations, so its ten lines
    of torch are called here on the same operations)"""
    t = torch.from_numpy(img.transpose((2, 0, 1))).float() / 255
    return torch.cat([torch.roll(t, shifts=list(s), dims=[1, 2]) for s in R.SHIFTS], dim=0)


def departures(ref_codes, feats64, codebook64):
    """fp64 distance from the best code to the code the fp32 reference chose, where they differ"""
    d = R.distances(feats64, codebook64)
    best = d.min(axis=1)
    chosen = d[np.arange(d.shape[0]), np.asarray(ref_codes).reshape(-1)]
    return chosen - best     # 0 where the reference took a nearest code


def replay_kmeans(km, X, X64, n_code, seed):
    """The matcher's k-means under `seed`, one reference iteration at a time (KMeans(max_iter=1).fit_predict from given
    centroids), each step's fp32 assignment and update set against fp64 on the same inputs."""
    torch.manual_seed(seed)
    init_idx = torch.randint(0, X.shape[0], size=[n_code]).numpy()      # the draw of init_methods._kpoints
    cents, errs, labels = [X[torch.from_numpy(init_idx)].clone()], [], None
    lowest_index, departure, dev = True, 0.0, 0.0
    for it in range(MAX_ITER):
        step = km.KMeans(n_clusters=n_code, max_iter=1, device=torch.device("cpu"))
        labels = step.fit_predict(X, centroids=cents[-1].clone())
        errs.append(float((step.centroids - cents[-1]).pow(2).sum()))
        cents.append(step.centroids.clone())
        prev64 = cents[-2].numpy().astype(np.float64)
        l64, c64, _, _ = R.kmeans_step(X64, prev64)
        departure = max(departure, float(departures(labels.numpy(), X64, prev64).max()))
        if np.array_equal(l64, labels.numpy()):
            dev = max(dev, float(np.abs(c64 - cents[-1].numpy()).max()))
        else:
            lowest_index = False
        if errs[-1] <= TOL:
            break
    clear = all(e >= 2 * TOL for e in errs[:-1]) and (errs[-1] <= TOL / 2 or (len(errs) == MAX_ITER and errs[-1] >= 2 * TOL))
    return {"init_idx": init_idx, "cents": cents, "errs": errs, "labels": labels, "lowest_index": lowest_index,
            "clear_stop": clear, "departure": departure, "dev_centroid": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vqnnf.npz"))
    args = ap.parse_args()
    tm, km = load_reference(args.reference)
    torch.set_num_threads(1)

    out, meta = {}, {"cases": [], "max_objects": 2}
    worst_departure, max_dist, dev_centroid, dev_fit, worst_aside = 0.0, 0.0, 0.0, 0.0, 0.0
    for name, seed, win_hw, box_hw, frame_xy, plant_xy in CASES:
        window, frame, box = make_case(seed, win_hw, box_hw, frame_xy, plant_xy)
        x, y, w, h = box
        tfeat = feats_of(frame)[:, y:y + h, x:x + w]                      # (27, rows, cols)
        X = tfeat.reshape(27, -1).transpose(1, 0)
        X64 = R.rect_features(frame, box)
        assert np.array_equal(X.numpy().astype(np.float64), X64)
        n_code = R.n_code_of(w, h)

        # The first seed from the case's own on whose run the reference's k-means (a) takes the lowest of equally near
        # centroids at every step, as its query-side assignment does — its fp32 matrix form breaks exact ties between
        # mirrored centroids either way, and no other implementation can follow that — (b) stops on an error a factor 2
        # from the tolerance at every step, and (c) runs three iterations or more.
        for kseed in range(seed, seed + 1000, 100):
            run = replay_kmeans(km, X, X64, n_code, kseed)
            if run["lowest_index"] and run["clear_stop"] and len(run["errs"]) >= 3:
                break
        else:
            raise AssertionError(f"{name}: no seed meets the conditions")
        init_idx, cents, errs, labels = run["init_idx"], run["cents"], run["errs"], run["labels"]
        n_iter = len(errs)
        worst_departure = max(worst_departure, run["departure"])
        dev_centroid = max(dev_centroid, run["dev_centroid"])
        torch.manual_seed(kseed)
        matcher = tm.VQNNFMatcher(template=tfeat, pca_dims=None, n_code=128, filters_cat="haar",
                                  filter_params={"kernel_size": 3, "sigma": 2, "n_scales": 3, "filters": 1}, verbose=False)
        assert matcher.n_code == n_code
        assert torch.equal(cents[-1], matcher.codebook), f"{name}: replayed k-means differs from the matcher's"
        # the whole fp64 run against the whole fp32 run: same stop, same labels, centroids apart by rounding only
        f_labels, f_cent, f_iter, _ = R.kmeans_fit(X64, init_idx)
        assert f_iter == n_iter and np.array_equal(f_labels, labels.numpy()), name
        dev_fit = max(dev_fit, float(np.abs(f_cent - cents[-1].numpy()).max()))

        # query side
        qfeat = feats_of(window)
        heat, _, _, _ = matcher.get_heatmap(qfeat)
        _, codes, _ = matcher.get_nnf(qfeat)
        codes = codes.numpy()
        Q64 = R.color_features(window).reshape(27, -1).T
        cb64 = matcher.codebook.numpy().astype(np.float64)
        dep = departures(codes, Q64, cb64)
        worst_departure = max(worst_departure, float(dep.max()))
        worst_aside = max(worst_aside, float((dep > 0).mean()))
        a64, gap64 = R.assign(Q64, cb64)
        off = codes.reshape(-1) != a64
        print(name, "query codes off the fp64 first minimum:", int(off.sum()), "largest gap there", float(gap64[off].max()) if off.any() else 0.0)
        max_dist = max(max_dist, float(R.distances(Q64, cb64).max()), float(R.distances(X64, cb64).max()))

        # filters, template responses, and the reference's convolutions evaluated in fp64 on the same code map
        fl = matcher.filtering_layer
        taps = np.stack([c.weight.data[0, 0].numpy() for c in fl.filters])
        dil = np.asarray([c.dilation for c in fl.filters], np.int64)
        ker = np.asarray(fl.scale_kernel_sizes, np.int64)
        wgt = np.asarray(fl.filter_weights, np.float64)
        tmpl = np.stack([t.reshape(-1).numpy() for t in fl.template_features])
        lab2d = labels.reshape(h, w)
        cw = torch.from_numpy(np.ones(n_code) / n_code)

        def integral64(c):
            return F.one_hot(c.long(), n_code).permute(2, 0, 1).double().cumsum(1).cumsum(2)[None]

        heat64, tmpl64 = torch.zeros(win_hw, dtype=torch.float64), []
        for conv, ks, fw in zip(fl.filters, fl.scale_kernel_sizes, fl.filter_weights):
            c64 = copy.deepcopy(conv).double()
            t = fl.forward_filter(integral64(lab2d), c64, ks, (1, 1))
            yq = fl.forward_filter(integral64(torch.from_numpy(codes)), c64, ks)
            sim = -(torch.abs(yq - t) * cw[None, :, None, None]).sum(dim=1).squeeze(0) * fw
            pl, pt = (win_hw[1] - sim.shape[1]) // 2, (win_hw[0] - sim.shape[0]) // 2
            heat64 += F.pad(sim, (pl, win_hw[1] - sim.shape[1] - pl, pt, win_hw[0] - sim.shape[0] - pt), value=sim.min().item())
            tmpl64.append(t.reshape(-1).numpy())
        heat64, tmpl64 = heat64.numpy(), np.stack(tmpl64)
        dev_heat = float(np.abs(heat64 - heat).max())
        dev_tmpl = float(np.abs(tmpl64 - tmpl).max())

        # the restatement agrees with that fp64 evaluation, and with the reference's descriptors
        r_taps, r_dil, r_ker, r_wgt = R.filter_bank(h, w)
        assert np.array_equal(r_taps, taps) and np.array_equal(r_dil, dil) and np.array_equal(r_ker, ker), name
        assert np.allclose(r_wgt, wgt, rtol=0, atol=1e-15)
        assert np.abs(R.template_responses(lab2d.numpy(), n_code, taps, dil, ker) - tmpl64).max() < 1e-9
        r_heat, _ = R.heatmap(codes, n_code, tmpl64, taps, dil, wgt)
        assert np.abs(r_heat - heat64).max() < 1e-9

        # peaks and boxes by the lines of vqnnf_template_matching.py:184-202,307, on the reference's heat map
        hm = heat.copy()
        pk, boxes = [], []
        query_w, query_h = box[3], box[2]
        for k in range(2):
            qx, qy = np.unravel_index(np.argmax(hm), hm.shape)
            pk.append((int(qx), int(qy)))
            top = hm[qx, qy]
            qx = int(qx + 1 - (R.odd(query_w) - 1) / 2)
            qy = int(qy + 1 - (R.odd(query_h) - 1) / 2)
            boxes.append((qy, qx, query_h, query_w))
            hm[qx:qx + query_w, qy:qy + query_h] = -0.82
            # no near-tie decides a peak: the runner-up outside the suppressed rectangle is 2 bars of check 4 away
            assert top - hm.max() > 2 * 4 * dev_heat, (name, k, top - hm.max(), dev_heat)
        # the first peak is the planted copy (a kernel of even size centres one pixel off)
        assert max(abs(boxes[0][0] - plant_xy[0]), abs(boxes[0][1] - plant_xy[1])) <= 1, (name, boxes, plant_xy)

        out.update({f"{name}/window": window, f"{name}/frame": frame, f"{name}/box": np.asarray(box, np.int32),
                    f"{name}/init_idx": init_idx.astype(np.int32), f"{name}/cent_1": cents[1].numpy(),
                    f"{name}/cent_2": cents[2].numpy(), f"{name}/cent_before_last": cents[-2].numpy(),
                    f"{name}/cent_last": cents[-1].numpy(), f"{name}/labels": labels.numpy().astype(np.uint8),
                    f"{name}/tmpl": tmpl, f"{name}/taps": taps, f"{name}/dil": dil.astype(np.int32),
                    f"{name}/ker": ker.astype(np.int32), f"{name}/wgt": wgt, f"{name}/codes": codes.astype(np.uint8),
                    f"{name}/heat": heat.astype(np.float32), f"{name}/peaks": np.asarray(pk, np.int32),
                    f"{name}/boxes": np.asarray(boxes, np.int32)})
        meta["cases"].append({"name": name, "kmeans_seed": kseed, "n_code": int(n_code), "n_iter": n_iter, "errors": errs, "dev_heat": dev_heat,
                              "dev_tmpl": dev_tmpl})
        print(name, "iters", n_iter, "dev_heat %.3e dev_tmpl %.3e" % (dev_heat, dev_tmpl), "peaks", pk, "boxes", boxes)

    # assignment: a pixel may differ from the fp64 arg-min only below eps_assign
    ulp = float(np.spacing(np.float32(max_dist)))
    meta["worst_departure"] = worst_departure
    meta["max_distance"] = max_dist
    meta["eps_assign"] = max(4 * worst_departure, 16 * ulp)
    meta["dev_centroid"] = dev_centroid
    meta["dev_fit"] = dev_fit
    # centroids lie in [0, 1]: a deviation beyond a few fp32 ulps of 1 would be a difference of method, not of rounding
    assert dev_centroid <= 16 * 2.0 ** -24 and dev_fit <= 64 * 2.0 ** -24, (dev_centroid, dev_fit)
    assert worst_aside <= 0.01, worst_aside
    for c in meta["cases"]:       # the share of pixels a test may set aside at that eps stays under 1 %
        n = c["name"]
        _, gap = R.assign(R.color_features(out[f"{n}/window"]).reshape(27, -1).T, out[f"{n}/cent_last"].astype(np.float64))
        c["near_tie_share"] = float((gap < meta["eps_assign"]).mean())
        assert c["near_tie_share"] <= 0.01, c

    # clip cosine: four pairs built from the first window (tests/test_vqnnf_gpu.py builds the same)
    devs = []
    for a, b in R.clip_pairs(out["a36x20/window"]):
        fa, fb = feats_of(a).reshape(1, -1), feats_of(b).reshape(1, -1)
        got = float(torch.nn.CosineSimilarity(dim=1)(fa, fb)[0])
        devs.append(abs(got - R.clip_cosine(a, b)))
    meta["dev_cosine"] = max(devs)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(args.out, **out)
    print(json.dumps({k: v for k, v in meta.items() if k != "cases"}), os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
