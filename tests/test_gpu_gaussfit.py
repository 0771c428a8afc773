"""The Gaussian-fit decoder on the GPU (include/esahrnet.h esahrnet_keypoints_gaussfit, csrc/keypoints_gaussfit.hip) against its
numpy restatement tests/gaussfit_ref.py on the same f32 planes: equal statuses and indices, the rows of rejected planes are those
of esahrnet_keypoints_ex, accepted fits are as deep as scipy's and as close to the analytic centre, a plane's bits depend on
neither its batch nor what the outputs held, the Hessian goes into esahrnet_correspondences(mode 1) as it is, and
net.keypoints_gaussfit is the forward followed by the decoder, on a side stream too.  Shapes: n = 2, K = 3, 32 x 40 (three
batches), and one 16 x 16 batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correspond_ref as R  # noqa: E402
import gaussfit_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

# The kernel and the restatement form every sum in the same order; they differ in `exp` (device library against numpy), at most
# an ulp per pixel.  On most fixture planes that leaves the two within 1e-14; where the one-ulp differences move a cost across
# the 1e-14 stopping rule, one of the two takes one more (tiny) step, and the distance is the size of that step.  Largest
# deviation over the accepted fixture planes, measured on an MI355X (the plane is noise+offset): centre
# 2.165e-11 px, (a, b, c) 4.426e-11.  The bounds are 4 x those: the fixtures are few, this is headroom for other seeds.
MEASURED_CENTRE = 2.165e-11
MEASURED_ABC = 4.426e-11


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet2, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, inference=inference, seg_hrnet2=seg_hrnet2, synth=synth)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(env, heat, fill=None, want_idx=True, want_fit=True, want_hess=True):
    """esahrnet_keypoints_gaussfit on a cuda tensor -> dict of cuda tensors; fill: a bit pattern every output byte holds first."""
    n, k, h, w = heat.shape
    out = dict(kp=torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), idx=torch.empty((n, k), dtype=torch.int32, device="cuda"),
               fit=torch.empty((n, k, 8), dtype=torch.float64, device="cuda"), status=torch.empty((n, k), dtype=torch.int32, device="cuda"),
               hess=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"))
    if fill is not None:
        for t in out.values():
            t.view(torch.uint8).fill_(fill)
    ptr = lambda name, want=True: out[name].data_ptr() if want else None       # noqa: E731
    env["L"].check(env["lib"].esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, h, w, ptr("kp"), ptr("idx", want_idx),
                                                          ptr("fit", want_fit), ptr("status"), ptr("hess", want_hess), _stream()))
    return out


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


@pytest.fixture(scope="module")
def fixtures(env):
    """The shared planes, the restatement's outputs (computed once) and the GPU's, per batch."""
    heat, names, truth = G.fixture_batches()
    res = {}
    for b, hm in heat.items():
        t = torch.from_numpy(hm).cuda()
        kp_ex, idx_ex = env["inference"]._keypoints(t, True)                  # esahrnet_keypoints_ex
        ref = G.gaussfit(hm, kp_ex.cpu().numpy())
        gpu = _raw(env, t)
        torch.cuda.synchronize()
        res[b] = dict(heat=hm, t=t, names=names[b], truth=truth[b], kp_ex=kp_ex, idx_ex=idx_ex, ref=ref,
                      gpu={k: v.cpu().numpy() for k, v in gpu.items()}, gpu_t=gpu)
    return res


# ---- 1. status, index, rejected rows ---------------------------------------------------------------------------------------------
def test_status_and_index_equal_the_restatement(fixtures):
    for b, f in fixtures.items():
        kp, idx, fit, status, hess = f["ref"]
        print(b, f["names"], "status", f["gpu"]["status"].ravel().tolist())
        assert f["gpu"]["status"].tolist() == status.tolist(), b
        assert f["gpu"]["idx"].tolist() == idx.tolist() == f["idx_ex"].cpu().tolist(), b
    st = dict(zip(fixtures["b"]["names"], fixtures["b"]["gpu"]["status"].ravel().tolist()))
    assert st["constant"] == 2 and st["nan"] == 3 and st["two-peaks"] in (0, 2)
    assert (fixtures["a"]["gpu"]["status"] == 0).all() and (fixtures["small"]["gpu"]["status"] == 0).all()
    # batch c: a centre outside the window (twice), a quadratic form that is not positive (twice), two accepted blobs
    assert fixtures["c"]["gpu"]["status"].ravel().tolist() == [2, 2, 2, 2, 0, 0]


def test_rejected_rows_are_those_of_keypoints_ex_and_nan(fixtures):
    seen = 0
    for b, f in fixtures.items():
        g = f["gpu_t"]
        rej = g["status"] != 0
        seen += int(rej.sum())
        assert _bits(g["kp"][rej], f["kp_ex"][rej]), b
        assert _bits(g["kp"][..., 2], f["kp_ex"][..., 2]), b                 # the peak is the raw maximum on every plane
        assert torch.isnan(g["fit"][rej]).all() and torch.isnan(g["hess"][rej]).all(), b
        acc = ~rej
        assert torch.isfinite(g["fit"][acc]).all(), b
        assert _bits(g["hess"][acc], -2.0 * g["fit"][acc][:, 3:6]), b
        assert _bits(g["kp"][acc][:, :2], g["fit"][acc][:, 1:3].to(torch.float32)), b
    assert seen >= 2


# ---- 2. accepted fits: depth, distance to the restatement, distance to the truth ------------------------------------------------
def test_accepted_fits_against_scipy_the_restatement_and_the_truth(fixtures):
    dev_c = dev_abc = 0.0
    for b, f in fixtures.items():
        hm = f["heat"].reshape((-1,) + f["heat"].shape[2:])
        fit, ref_fit = f["gpu"]["fit"].reshape(-1, 8), f["ref"][2].reshape(-1, 8)
        status, idx = f["gpu"]["status"].ravel(), f["gpu"]["idx"].ravel()
        for i, name in enumerate(f["names"]):
            if status[i] != 0:
                continue
            x_ref, c_ref, _ = G.scipy_fit(hm[i], int(idx[i]))
            r = G.model_residuals(fit[i, :7], hm[i], int(idx[i]))
            c = float(r @ r)
            dc, dabc = float(np.abs(fit[i, 1:3] - ref_fit[i, 1:3]).max()), float(np.abs(fit[i, 3:6] - ref_fit[i, 3:6]).max())
            dev_c, dev_abc = max(dev_c, dc), max(dev_abc, dabc)
            line = f"{b}/{name}: cost {c:.6e} scipy {c_ref:.6e}; to the restatement: centre {dc:.3e} px, (a, b, c) {dabc:.3e}"
            tr = f["truth"][i]
            if tr is not None:                                                 # a noise-free blob: the analytic centre
                e, e_ref = np.hypot(fit[i, 1] - tr[0], fit[i, 2] - tr[1]), np.hypot(x_ref[1] - tr[0], x_ref[2] - tr[1])
                line += f"; centre error {e:.3e} px, scipy {e_ref:.3e} px"
            print(line)
            assert c <= c_ref * (1 + 1e-6) + 1e-12, (name, c, c_ref)          # tests/test_correspond_host.py's bound
            assert abs(fit[i, 7] - c) <= 1e-9 * c + 1e-20, name
            if tr is not None:
                assert e <= 2 * e_ref + 1e-6, (name, e, e_ref)
    print(f"largest deviation from the restatement: centre {dev_c:.3e} px, (a, b, c) {dev_abc:.3e}")
    assert dev_c <= 4 * MEASURED_CENTRE and dev_abc <= 4 * MEASURED_ABC


# ---- 3. a plane's bits depend on neither its batch nor what the outputs held ----------------------------------------------------
def test_a_plane_alone_in_a_batch_and_in_a_permuted_batch(env, fixtures):
    for b in ("a", "b", "c"):
        f = fixtures[b]
        t, g = f["t"], f["gpu_t"]
        flat = t.reshape(1, 6, G.H, G.W)
        perm = torch.tensor([4, 2, 0, 5, 1, 3], device="cuda")
        gp = _raw(env, flat[:, perm].contiguous())
        for i in range(6):
            one = _raw(env, flat[:, i:i + 1].contiguous())
            for key in ("kp", "idx", "fit", "status", "hess"):
                whole = g[key].reshape((1, 6) + g[key].shape[2:])
                assert _bits(one[key], whole[:, i:i + 1]), (b, i, key)
        for key in ("kp", "idx", "fit", "status", "hess"):
            whole = g[key].reshape((1, 6) + g[key].shape[2:])
            assert _bits(gp[key], whole[:, perm]), (b, key)


@pytest.mark.parametrize("fill", [0xFF, 0x7F, 0x00])
def test_outputs_prefilled_with_patterns_give_the_same_bits(env, fixtures, fill):
    """0xFF bytes: NaN in f32 and f64, -1 as an index; 0x7F: NaN as well, a huge index.  Also with the optional outputs left out:
    without idx_dev the index passes through status_dev."""
    for b, f in fixtures.items():
        g = f["gpu_t"]
        again = _raw(env, f["t"], fill=fill)
        for key in ("kp", "idx", "fit", "status", "hess"):
            assert _bits(again[key], g[key]), (b, key)
        bare = _raw(env, f["t"], fill=fill, want_idx=False, want_fit=False, want_hess=False)
        assert _bits(bare["kp"], g["kp"]) and _bits(bare["status"], g["status"]), b
        for key in ("idx", "fit", "hess"):                                    # not written
            assert (bare[key].view(torch.uint8) == fill).all(), (b, key)


# ---- 4. the Hessian is the one esahrnet_correspondences(mode 1) takes ------------------------------------------------------------
def test_hessian_feeds_the_correspondences_as_it_is(env, fixtures):
    inf = env["inference"]
    for b in ("a", "b", "c"):
        f = fixtures[b]
        g = f["gpu_t"]
        m, k = 2, 3
        boxes = torch.tensor([[100, 50, 356, 306], [400, 300, 700, 600]], dtype=torch.int32, device="cuda")
        rates = torch.tensor([1.0, 256 / 300], dtype=torch.float64, device="cuda")
        valid = torch.ones(m, dtype=torch.int32, device="cuda")
        count, order, pts, w = inf.keypoints_to_correspondences(g["kp"], boxes, rates, valid, hess=g["hess"], thresh=0.0, min_k=k,
                                                                weights="hessian")
        torch.cuda.synchronize()
        fit = f["gpu"]["fit"]
        hess = -2.0 * fit[..., 3:6]                                           # rate (2 [[a, b], [b, c]])^(1/2) = rate (-hess)^(1/2)
        ec, eo, ep, ew = R.record(f["gpu"]["kp"], boxes.cpu().numpy(), rates.cpu().numpy(), valid.cpu().numpy(), 0.0, k, hess)
        gw = w.cpu().numpy()
        assert count.cpu().tolist() == ec.tolist() and order.cpu().tolist() == eo.tolist()
        assert np.array_equal(gw == 0, ew == 0)
        assert np.all(np.abs(gw - ew) <= 4 * np.spacing(np.abs(ew)))          # tests/test_gpu_correspond.py's tolerance
        rejected = f["gpu"]["status"] != 0
        for i in range(m):
            for j in range(int(ec[i])):
                zero = (gw[i, j] == 0).all()
                assert zero == bool(rejected[i, eo[i, j]]), (b, i, j)           # a rejected keypoint: a point without a weight
                if not zero:                                                   # w w = rate^2 * 2 [[a, b], [b, c]]
                    a, bb, c = fit[i, eo[i, j], 3:6]
                    wxx, wxy, wyy = gw[i, j]
                    sq = np.array([wxx * wxx + wxy * wxy, wxy * (wxx + wyy), wxy * wxy + wyy * wyy])
                    want = float(rates[i]) ** 2 * 2.0 * np.array([a, bb, c])
                    assert np.allclose(sq, want, rtol=1e-12, atol=1e-15), (b, i, j)


# ---- 5. the forward, then the decoder ---------------------------------------------------------------------------------------------
def test_net_keypoints_gaussfit_is_the_forward_then_the_decoder(env, golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_hrnet2_64.npz"), allow_pickle=False)
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=tuple(int(v) for v in g["widths"])))
    sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=int(g["seed"]))
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    x = env["synth"].make_crops(int(g["n"]), 1, int(g["hw"]), int(g["hw"]), seed=int(g["seed"])).cuda()
    with torch.no_grad():
        kp, fit, status, hess = net.keypoints_gaussfit(x, return_fit=True)
        kp3, status3, hess3 = net.keypoints_gaussfit(x)
        heat = net(x)
        rkp, rfit, rstatus, rhess = env["inference"].gaussfit_keypoints(heat)
        kp_ex = env["inference"].heatmaps_to_keypoints(heat)
    torch.cuda.synchronize()
    # once more under a stream that is not the default one, with the input produced on it: forward and decoder must both
    # follow the caller's current stream (nothing here waits for the side stream before the results are read on it)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        xs = x * 1.0                                                          # enqueued on the side stream
        skp, sfit, sstatus, shess = net.keypoints_gaussfit(xs, return_fit=True)
        packed = torch.cat([skp.double().flatten(), sfit.flatten(), sstatus.double().flatten(), shess.flatten()])
        host = packed.to("cpu", non_blocking=False)                           # a copy on the side stream, then its own wait
    want = torch.cat([kp.double().flatten(), fit.flatten(), status.double().flatten(), hess.flatten()]).cpu()
    assert torch.equal(host.view(torch.int64), want.view(torch.int64))
    torch.cuda.synchronize()
    assert _bits(kp, rkp) and _bits(fit, rfit) and torch.equal(status, rstatus) and _bits(hess, rhess)
    assert _bits(kp3, rkp) and torch.equal(status3, rstatus) and _bits(hess3, rhess)
    rej = status != 0
    assert _bits(kp[rej], kp_ex[rej]) and _bits(kp[..., 2], kp_ex[..., 2])
    print("tiny_hrnet2_64: statuses", np.bincount(status.cpu().numpy().ravel(), minlength=4).tolist())
    from esa_pose_estimation_amd import inference
    sx, sy, th = inference.gaussfit_sigma_theta(fit)
    ok = (status == 0).cpu().numpy()
    assert np.isfinite(sx[ok]).all() and np.all(sx[ok] >= sy[ok]) and np.isnan(sx[~ok]).all()


# ---- 6. the statistical property ---------------------------------------------------------------------------------------------------
def test_fitted_sigma_is_closer_to_the_truth_than_the_final2_hessian(env):
    """tests/test_gaussfit_host.py asserts the same ordering with the two restatements; here both figures come from the GPU."""
    planes, true = G.aniso_planes()
    t = torch.from_numpy(planes).cuda()
    _, fit, status, _ = env["inference"].gaussfit_keypoints(t)
    _, hess = env["inference"].heatmaps_to_keypoints(t, refine="get_final2", return_hessian=True)
    torch.cuda.synchronize()
    assert (status == 0).all()
    fit, h = fit.cpu().numpy().reshape(-1, 8), hess.cpu().numpy().reshape(-1, 3)
    assert np.isfinite(h).all()
    e_fit = G.sigma_error(np.stack(G.sigma_of(fit[:, 3], fit[:, 4], fit[:, 5]), 1), true)
    det = h[:, 0] * h[:, 2] - h[:, 1] ** 2
    e_f2 = G.sigma_error(np.stack([-h[:, 2] / det - 4.0, h[:, 1] / det, -h[:, 0] / det - 4.0], 1), true)
    print(f"median relative error of Sigma: fit {np.median(e_fit):.3e}, get_final2 Hessian {np.median(e_f2):.3e}")
    assert np.median(e_fit) <= np.median(e_f2)
