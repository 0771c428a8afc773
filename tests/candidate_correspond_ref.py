"""Numpy restatement of the candidates' device stage (include/esahrnet.h esahrnet_correspondences_cand, csrc/correspond.hip:
correspond_cand_kernel), shared by tests/test_candidate_correspond_host.py and tests/test_gpu_candidate_correspond.py.

Every quantity of the record is either copied or one f64 product, one f64 sum, a division or a square root, each a numpy scalar
operation that rounds once: the record is compared bit for bit.  corr_hessian_weight (csrc/correspond.h) is restated here, not
borrowed from the package."""
import numpy as np

f64 = np.float64


def hessian_weight(H, rate):
    """H = (dxx, dxy, dyy) -> rate * (-H)^(1/2) as (wxx, wxy, wyy); zeros where -H is not positive definite, holds a NaN or the
    weight is not finite.  A = -H = [[a, b], [b, c]]: s = sqrt(det A), t = sqrt((a + c) + 2 s), A^(1/2) = (A + s I) / t."""
    a, b, c, rate = -f64(H[0]), -f64(H[1]), -f64(H[2]), f64(rate)
    with np.errstate(all="ignore"):
        ac = a * c
        bb = b * b
        det = ac - bb
        if not (a > 0.0 and det > 0.0):
            return np.zeros(3)
        s = np.sqrt(det)
        two_s = f64(2.0) * s
        t = np.sqrt((a + c) + two_s)
        w = np.array([rate * ((a + s) / t), rate * (b / t), rate * ((c + s) / t)])
    return w if np.isfinite(w).all() else np.zeros(3)


def to_image(p, inv, origin):
    """val.py:180 for one coordinate: the product rounded, then the sum."""
    with np.errstate(all="ignore"):
        scaled = f64(p) * inv
        return scaled + f64(origin)


def record(cand, hess, crop_boxes, rates, valid, thresh, min_k, mode):
    """cand f32 [m,K,M,3], hess f64 [m,K,M,3] or None (mode 0), crop_boxes int [m,4], rates f64 [m], valid int [m] ->
    dict(cpts f64 [m,K,M,2], cw f64 [m,K,M,3], cpeak f32 [m,K,M], count int32 [m], order int32 [m,K])."""
    cand = np.asarray(cand, np.float32)
    m, k, M = cand.shape[:3]
    out = dict(cpts=np.zeros((m, k, M, 2)), cw=np.zeros((m, k, M, 3)), cpeak=np.zeros((m, k, M), np.float32),
               count=np.zeros(m, np.int32), order=np.full((m, k), -1, np.int32))
    for c in range(m):
        if not valid[c]:
            continue
        peaks = cand[c, :, 0, 2]
        numbers = [j for j in range(k) if not np.isnan(peaks[j])]                   # a NaN primary peak is never selected
        above = sum(bool(f64(peaks[j]) > thresh) for j in numbers)
        cnt = min(max(above, min_k), len(numbers))
        ranked = sorted(numbers, key=lambda j: (-float(peaks[j]), j))               # largest first, equal peaks by lower index
        with np.errstate(all="ignore"):
            inv = f64(1.0) / f64(rates[c])
        for i, j in enumerate(ranked[:cnt]):
            out["order"][c, i] = j
            for mm in range(M):
                x, y, pk = cand[c, j, mm]
                out["cpeak"][c, i, mm] = pk
                if np.isfinite(x) and np.isfinite(y):
                    out["cpts"][c, i, mm] = (to_image(x, inv, crop_boxes[c][0]), to_image(y, inv, crop_boxes[c][1]))
                    out["cw"][c, i, mm] = hessian_weight(hess[c, j, mm], rates[c]) if mode else (f64(pk), 0.0, f64(pk))
                else:
                    out["cpts"][c, i, mm] = np.nan
        out["count"][c] = cnt
    return out


CAMERA = np.array([[3003.41297, 0.0, 960.0], [0.0, 3003.41297, 600.0], [0.0, 0.0, 1.0]])


def random_hessians(rng, cand):
    """A Hessian per candidate row, f64 [.., 3] = (dxx, dxy, dyy): negative definite with a random axis ratio and tilt; NaN where
    the candidate's row is NaN; every 7th one a saddle, every 11th zero, every 13th NaN (counted over the flattened rows)."""
    shape = cand.shape[:-1]
    n = int(np.prod(shape))
    a, c = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    b = rng.uniform(-0.9, 0.9, n) * np.sqrt(a * c)
    H = -np.stack([a, b, c], 1)
    i = np.arange(n)
    H[i % 7 == 3] *= [1.0, 1.0, -1.0]                      # indefinite
    H[i % 11 == 5] = 0.0
    H[i % 13 == 9] = np.nan
    H[np.isnan(cand.reshape(n, 3)[:, 0])] = np.nan
    return H.reshape(*shape, 3)


def random_scene(rng, n, k, nbad, M=4, noise=0.3, side=256.0):
    """n images of a k-keypoint model under random poses, as candidate rows in crop coordinates: -> dict(kp3d [k,3], K, cand f32
    [n,k,M,3], crop_boxes int32 [n,4], rates f64 [n], bad [n][nbad]).  `bad` keypoints have their primary displaced by 30-120 image
    pixels; the true place is the LAST-but-one finite candidate, with 0.5-0.95 of the primary's peak; with M >= 3 every second bad
    keypoint has, in front of it, a runner-up at the true place with 0.05-0.25 of the primary's peak (below any sensible
    min_ratio).  Half of the good keypoints carry a decoy runner-up 30-120 px away.  The remaining rows are the NaN rows of "no
    further peak".  Primary peaks are finite."""
    from esa_pose_estimation_amd import pnp
    far = lambda m: rng.uniform(30, 120, (m, 2)) * rng.choice([-1, 1], (m, 2))     # noqa: E731
    kp3d = rng.uniform(-0.6, 0.6, (k, 3))
    cand = np.full((n, k, M, 3), np.nan, np.float32)
    boxes = np.zeros((n, 4), np.int32)
    rates = np.zeros(n)
    bads = []
    for i in range(n):
        R = pnp.rodrigues(rng.uniform(-1.2, 1.2, 3))
        t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(5.0, 12.0)])
        true = pnp.project(kp3d, R, t, CAMERA) + rng.normal(0, noise, (k, 2))
        peak = rng.uniform(0.3, 1.0, k)
        bad = np.sort(rng.choice(k, nbad, replace=False)) if nbad else np.zeros(0, np.int64)
        good = np.setdiff1d(np.arange(k), bad)
        decoy = rng.choice(good, len(good) // 2, replace=False)
        rows = np.full((k, M, 3), np.nan)
        rows[:, 0, :2], rows[:, 0, 2] = true, peak
        rows[bad, 0, :2] += far(len(bad))
        if M > 1:
            for a, j in enumerate(bad):
                slot = 1
                if M >= 3 and a % 2:
                    rows[j, 1] = (*(true[j] + rng.normal(0, 0.2, 2)), peak[j] * rng.uniform(0.05, 0.25))
                    slot = 2
                rows[j, slot] = (*true[j], peak[j] * rng.uniform(0.5, 0.95))
            rows[decoy, 1, :2] = true[decoy] + far(len(decoy))
            rows[decoy, 1, 2] = peak[decoy] * rng.uniform(0.3, 0.95, len(decoy))
        pts = rows[..., :2].reshape(-1, 2)
        pts = pts[np.isfinite(pts[:, 0])]
        x0, y0 = int(pts[:, 0].min()) - 20, int(pts[:, 1].min()) - 20
        rate = side / (max(np.ptp(pts[:, 0]), np.ptp(pts[:, 1])) + 40.0)
        rows[..., :2] = (rows[..., :2] - [x0, y0]) * rate
        cand[i] = rows
        boxes[i] = (x0, y0, x0 + int(side / rate), y0 + int(side / rate))
        rates[i] = rate
        bads.append(bad)
    return dict(kp3d=kp3d, K=CAMERA, cand=cand, crop_boxes=boxes, rates=rates, bad=bads)


FIELDS = ("cpts", "cw", "cpeak", "count", "order")


def same_bits(a, b):
    """Equal as bytes: NaN payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
