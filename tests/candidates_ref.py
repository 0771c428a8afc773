"""Numpy oracle of the candidate decoder (include/esahrnet.h esahrnet_keypoints_candidates, csrc/keypoints_candidates.hip), and
the planes tests/test_gpu_candidates.py runs it on.

Rank 0 is np.argmax of the flattened plane (first maximum, first NaN).  Rank m >= 1 is the largest value among the pixels that
are neither NaN nor -inf, are >= each of their 8 neighbours (outside the plane: ignored; NaN: disqualifies) and lie at Chebyshev
distance > r from every earlier candidate; ties to the lower flat index; none left: NaN x 3 and index -1 from there on.  The
sub-pixel step is oracle.keypoints_ref.refine_one at the candidate's pixel on the plane clamped at 1e-10, the peak the raw value."""
import numpy as np

from oracle.keypoints_ref import refine_one


def local_maxima(plane):
    """bool [H,W]: conditions (a) and (b)."""
    h, w = plane.shape
    pad = np.full((h + 2, w + 2), -np.inf, plane.dtype)
    pad[1:-1, 1:-1] = plane
    ok = ~np.isnan(plane) & (plane != -np.inf)
    with np.errstate(invalid="ignore"):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    ok &= plane >= pad[dy:dy + h, dx:dx + w]              # a NaN neighbour compares False
    return ok


def candidates_plane(plane, M, r):
    """plane f32 [H,W] -> cand f32 [M,3], idx int32 [M]."""
    h, w = plane.shape
    clamped = np.maximum(plane, np.float32(1e-10))
    cand = np.full((M, 3), np.nan, np.float32)
    idx = np.full(M, -1, np.int32)
    ys, xs = np.mgrid[0:h, 0:w]
    free = local_maxima(plane)
    for m in range(M):
        if m == 0:
            i = int(np.argmax(plane.ravel()))
        else:
            if not free.any():
                break
            i = int(np.argmax(np.where(free, plane, -np.inf).ravel()))
        py, px = divmod(i, w)
        cand[m, :2] = refine_one(clamped, np.array([px, py], np.float32))
        cand[m, 2] = plane[py, px]
        idx[m] = i
        free = free & (np.maximum(np.abs(ys - py), np.abs(xs - px)) > r)
    return cand, idx


def candidates(hm, M, r):
    """hm f32 [N,K,H,W] -> cand f32 [N,K,M,3], idx int32 [N,K,M]."""
    n, k = hm.shape[:2]
    cand = np.empty((n, k, M, 3), np.float32)
    idx = np.empty((n, k, M), np.int32)
    for a in range(n):
        for b in range(k):
            cand[a, b], idx[a, b] = candidates_plane(hm[a, b], M, r)
    return cand, idx


# ---- the planes ------------------------------------------------------------------------------------------------------------------
def _blobs(h, w, spots, sigma=1.5):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.zeros((h, w))
    for cx, cy, amp in spots:
        g += amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sigma * sigma))
    return g


SHOULDER = [(5, 6), (5, 7), (5, 8), (5, 9)]               # (row, column): the pixels of "shoulder" that decrease away from its peak
RING = dict(peak=(2, 2), twin=(2, 3), d2=(4, 2), d6=(2, 8), d7=(9, 3))     # "ring": runner-ups at Chebyshev 1, 2, 6 and 7 of the peak

NAMES = ("two-blobs", "three-blobs", "corner-edge", "constant", "twins", "ring", "shoulder", "one-nan", "nan-neighbour",
         "all-neg-inf", "noisy", "all-nan")


def planes(h, w, seed=0):
    """The twelve planes of NAMES at h x w (15 x 16 at least), f32 [12,h,w]."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    out = []
    out.append(_blobs(h, w, [(4.3, 5.2, 1.0), (w - 5.6, h - 4.7, 0.7)]))
    out.append(_blobs(h, w, [(w - 4.4, 3.8, 1.0), (3.7, h - 4.2, 0.8), (w / 2 + 0.3, h / 2 - 0.4, 0.6)]))
    out.append(_blobs(h, w, [(0.3, 0.4, 1.0), (w - 1.0, h / 2 + 0.2, 0.8)]))                # a corner, the right edge
    out.append(np.full((h, w), 0.25))
    p = np.full((h, w), 0.1)                                                               # twins: equal single pixels
    p[2, 3] = p[12, 11] = 1.0
    out.append(p)
    p = np.zeros((h, w))
    for name, v in (("peak", 1.0), ("twin", 1.0), ("d2", 0.9), ("d6", 0.8), ("d7", 0.6)):
        p[RING[name]] = v
    out.append(p)
    p = np.zeros((h, w))
    p[5, 5] = 1.0
    for i, rc in enumerate(SHOULDER):
        p[rc] = 0.9 - 0.1 * i
    out.append(p)
    p = _blobs(h, w, [(5.4, 4.6, 1.0)]) + 0.05
    p[h - 3, w - 4] = np.nan
    out.append(p)
    p = np.full((h, w), 0.05)                                  # the 0.7 spike has a NaN neighbour: never a candidate
    p[3, 3], p[10, 10], p[10, 11] = 1.0, 0.7, np.nan
    out.append(p)
    out.append(np.full((h, w), -np.inf))
    out.append(_blobs(h, w, [(5.1, 8.3, 0.8), (w - 5.2, h - 5.5, 0.5)], sigma=2.0) + 0.1 + 0.02 * rng.standard_normal((h, w)))
    out.append(np.full((h, w), np.nan))
    return np.stack(out).astype(np.float32)


# ---- end to end: heat-maps whose global maximum sits on the wrong blob for two keypoints per image -------------------------------
def wrong_blob_scene(n=4, k=11, size=64, nbad=2, seed=0):
    """n images of a k-keypoint model under known poses, as size x size heat-map centres: -> dict(kp3d, K, poses [(R, t)], boxes
    [(x0, y0)], rates, centers f32 [n,k,2] the true keypoints in heat-map pixels, wrong f32 [n,k,2] where keypoint j's higher,
    wrong blob sits (NaN: none), bad [n][nbad]).  Every true keypoint is at least 5 px inside the map; a wrong blob is at least
    14 px (Chebyshev) from its keypoint's true place, i.e. tens of image pixels."""
    from esa_pose_estimation_amd import pnp, synth
    rng = np.random.default_rng(seed)
    K = synth.ESA_CAMERA
    kp3d = rng.uniform(-0.6, 0.6, (k, 3))
    centers = np.empty((n, k, 2), np.float32)
    wrong = np.full((n, k, 2), np.nan, np.float32)
    poses, boxes, rates, bads = [], [], [], []
    for i in range(n):
        R = pnp.rodrigues(rng.uniform(-1.2, 1.2, 3))
        t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(5.0, 12.0)])
        uv = pnp.project(kp3d, R, t, K)
        side = max(np.ptp(uv[:, 0]), np.ptp(uv[:, 1])) * 1.25
        x0, y0 = (int((uv[:, d].min() + uv[:, d].max() - side) / 2) for d in (0, 1))
        rate = size / side
        c = (uv - [x0, y0]) * rate
        assert c.min() >= 5 and c.max() <= size - 6, (c.min(), c.max())
        bad = np.sort(rng.choice(k, nbad, replace=False))
        for j in bad:
            while True:
                p = rng.uniform(6, size - 7, 2)
                if np.abs(p - c[j]).max() >= 14:
                    break
            wrong[i, j] = p
        centers[i] = c
        poses.append((R, t)); boxes.append((x0, y0)); rates.append(rate); bads.append(bad)
    return dict(kp3d=kp3d, K=K, poses=poses, boxes=boxes, rates=rates, centers=centers, wrong=wrong, bad=bads)


def wrong_blob_heatmaps(scene, size=64):
    """synth.render_heatmaps of the scene: amplitude 1.0 at the wrong place and 0.7 at the true place where there is a wrong
    blob, a single blob of amplitude 1.0 elsewhere.  -> f32 torch [n,k,size,size] (CPU)."""
    import torch
    from esa_pose_estimation_amd import synth
    true = synth.render_heatmaps(torch.from_numpy(scene["centers"]), size)
    has = torch.from_numpy(~np.isnan(scene["wrong"][..., 0]))[..., None, None]
    other = synth.render_heatmaps(torch.from_numpy(np.nan_to_num(scene["wrong"])), size)
    return torch.where(has, other + 0.7 * true, true).contiguous()


def check_wrong_blob_poses(scene, cand):
    """What the end-to-end test asserts on the candidates cand [n,k,M,3] of wrong_blob_heatmaps(scene), from either decoder."""
    from esa_pose_estimation_amd import pnp
    a = (scene["kp3d"], scene["K"], scene["boxes"], scene["rates"])
    q, t, used = pnp.candidates_to_pose_batch(cand, *a, thresh=0.5, min_k=0)
    q1, t1, used1 = pnp.candidates_to_pose_batch(cand[:, :, :1], *a, thresh=0.5, min_k=0)
    for i, (R, tt) in enumerate(scene["poses"]):
        want = np.zeros(cand.shape[1], np.int32)
        want[scene["bad"][i]] = 1
        assert np.array_equal(used[i], want), (i, used[i], scene["bad"][i])
        assert (used1[i] == 0).all()
        qt = pnp.rotation_to_quat_wxyz(R)
        s, s1 = pnp.speed_score(q[i], t[i], qt, tt)[0], pnp.speed_score(q1[i], t1[i], qt, tt)[0]
        print(f"image {i}: SPEED with one candidate {s1:.5f}, with runner-ups {s:.6f}")
        assert s < 0.05, (i, s)                        # the no-outlier bound of tests/test_pnp_native.py
        assert s1 > s, (i, s1, s)
