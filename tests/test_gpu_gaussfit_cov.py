"""The covariance of the Gaussian fit's centre on the GPU (include/esahrnet.h esahrnet_keypoints_gaussfit_cov,
esahrnet_forward_keypoints_gaussfit_cov, esahrnet_frames_keypoints_gaussfit_cov): kp, idx, fit, status and hess bit-identical to
the siblings without _cov; cov and info independent of the batch and of what the outputs held; cov held to scipy's
least_squares through the numpy restatement tests/gaussfit_cov_ref.py (which differs from the kernel in exp alone); info the
header's three lines on the GPU's own cov; the weights esahrnet_correspondences(mode 1) makes of info; the three fused forms
against esahrnet_forward + the stand-alone entry; the loader; and pipeline.estimate_poses(weights="covariance")."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correspond_ref as R  # noqa: E402
import gaussfit_cov_ref as V  # noqa: E402
import gaussfit_ref as G  # noqa: E402
import test_gpu_gaussfit_forward as F  # noqa: E402  (its nets, its blob heat-maps, its scene)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_bits = F._bits
NAMES16 = ["n-aniso", "n-aniso+offset", "n-sharp", "n-border", "n-corner", "clean", "constant", "outside", "nan"]
ACCEPTED16 = NAMES16[:6]
OUTS = ("kp", "idx", "fit", "status", "hess", "cov", "info")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, inference, pipeline, pnp, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, inference=inference, pipeline=pipeline, pnp=pnp, synth=synth,
                seg_hrnet=seg_hrnet, seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


@pytest.fixture(scope="module")
def planes():
    """The host test's fixtures and the guard cases: "p16" f32 [3, 3, 16, 16] (NAMES16 in order), "p40" f32 [1, 1, 40, 40]
    (the sigma-3 blob, which needs room) and "p6" f32 [1, 1, 2, 3] (n = 6 < 7 parameters), each with the restatement's and
    least_squares' results, computed once."""
    guard = V.guard_planes()
    p16 = np.stack([V.noisy_plane(n) if n in V.NOISY else guard[n] for n in NAMES16]).reshape(3, 3, 16, 16)
    out = {"p16": p16, "p40": V.noisy_plane("n-wide").reshape(1, 1, 40, 40), "p6": G.blob(2, 3, 1.2, 0.6, 1.0, 1.0, 0.0)[0].reshape(1, 1, 2, 3)}
    ref = {k: V.gaussfit_cov(v) for k, v in out.items()}
    lsq = {}
    for key, names in (("p16", NAMES16), ("p40", ["n-wide"])):
        flat = out[key].reshape((-1,) + out[key].shape[2:])
        lsq[key] = [V.lsq_pcov(pl, int(np.argmax(pl))) if n in V.NOISY else None for pl, n in zip(flat, names)]
    return out, ref, lsq


def _call(env, heat, cov=True, info=True, floor=V.COV_FLOOR, fill=0xFF, sibling=False):
    """esahrnet_keypoints_gaussfit_cov (or its sibling) on buffers of the test's own, pre-filled with `fill` bytes -> dict of
    tensors (cov / info stay as pre-filled when not passed)."""
    lib, L = env["lib"], env["L"]
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    o = dict(kp=torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), idx=torch.empty((n, k), dtype=torch.int32, device="cuda"),
             fit=torch.empty((n, k, 8), dtype=torch.float64, device="cuda"), status=torch.empty((n, k), dtype=torch.int32, device="cuda"),
             hess=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"), cov=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"),
             info=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"))
    for t in o.values():
        t.view(torch.uint8).fill_(fill)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if sibling:
        L.check(lib.esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, h, w, o["kp"].data_ptr(), o["idx"].data_ptr(), o["fit"].data_ptr(),
                                                o["status"].data_ptr(), o["hess"].data_ptr(), st))
    else:
        L.check(lib.esahrnet_keypoints_gaussfit_cov(heat.data_ptr(), n, k, h, w, o["kp"].data_ptr(), o["idx"].data_ptr(),
                                                    o["fit"].data_ptr(), o["status"].data_ptr(), o["hess"].data_ptr(),
                                                    o["cov"].data_ptr() if cov else None, o["info"].data_ptr() if info else None,
                                                    float(floor), st))
    torch.cuda.synchronize()
    return o


def _untouched(t, fill=0xFF):
    return bool((t.view(torch.uint8) == fill).all())


# ---- 1. the stand-alone entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p16", "p40", "p6"])
def test_fit_outputs_are_the_siblings_bits(env, planes, key):
    """kp, idx, fit, status, hess of the _cov entry against esahrnet_keypoints_gaussfit: the same bits with both new outputs,
    with either alone and with neither; a pointer that is NULL is not written; and the Python form returns the same."""
    heat = torch.from_numpy(planes[0][key]).cuda()
    sib = _call(env, heat, sibling=True)
    both = _call(env, heat)
    for cov, info in ((True, True), (True, False), (False, True), (False, False)):
        got = _call(env, heat, cov=cov, info=info)
        for name in OUTS[:5]:
            assert _bits(got[name], sib[name]), (name, cov, info)
        assert _bits(got["cov"], both["cov"]) if cov else _untouched(got["cov"])
        assert _bits(got["info"], both["info"]) if info else _untouched(got["info"])
    py = env["inference"].gaussfit_keypoints(heat, return_cov=True)
    old = env["inference"].gaussfit_keypoints(heat)
    torch.cuda.synchronize()
    assert len(py) == 6 and len(old) == 4
    for a, name in zip(py, ("kp", "fit", "status", "hess", "cov", "info")):
        assert _bits(a, both[name]), name
    for a, name in zip(old, ("kp", "fit", "status", "hess")):
        assert _bits(a, sib[name]), name


def test_statuses_and_guards(env, planes):
    """The statuses are the restatement's; cov and info are NaN x 3 exactly where the restatement's are: a rejected fit
    (constant plane, centre outside the window), a NaN in the window, and n = 6 pixels (dof <= 0).  The noise-free blob has a
    finite covariance below the reference's floor: info NaN with the default floor, finite with floor 0."""
    heat, ref, _ = planes
    for key in heat:
        got = _call(env, torch.from_numpy(heat[key]).cuda())
        st, _, cov, info = ref[key]
        if key != "p6":                         # 6 pixels, 7 parameters: the fit is not determined, its status says nothing
            assert got["status"].cpu().numpy().tolist() == st.tolist(), key
        assert np.array_equal(np.isnan(got["cov"].cpu().numpy()), np.isnan(cov)), key
        assert np.array_equal(np.isnan(got["info"].cpu().numpy()), np.isnan(info)), key
    got = _call(env, torch.from_numpy(heat["p16"]).cuda())
    cov, info, st = (got[n].cpu().numpy().reshape(9, -1) for n in ("cov", "info", "status"))
    for i, name in enumerate(NAMES16):
        if name in V.NOISY:
            assert st[i] == 0 and np.isfinite(cov[i]).all() and np.isfinite(info[i]).all() and cov[i, 0] > 1e-6, name
    i = NAMES16.index("clean")
    assert st[i] == 0 and np.isfinite(cov[i]).all() and 0 < cov[i, 0] < 1e-6 and 0 < cov[i, 2] < 1e-6 and np.isnan(info[i]).all()
    for name, s in (("constant", 2), ("outside", 2), ("nan", 3)):
        i = NAMES16.index(name)
        assert st[i] == s and np.isnan(cov[i]).all() and np.isnan(info[i]).all(), name
    zero = _call(env, torch.from_numpy(heat["p16"]).cuda(), floor=0.0)
    assert _bits(zero["cov"], got["cov"])
    assert np.isfinite(zero["info"].cpu().numpy().reshape(9, 3)[NAMES16.index("clean")]).all()
    six = _call(env, torch.from_numpy(heat["p6"]).cuda())
    assert bool(torch.isnan(six["cov"]).all()) and bool(torch.isnan(six["info"]).all())


def test_cov_and_info_do_not_depend_on_the_batch_or_on_the_outputs_contents(env, planes):
    """The same bits for a plane alone, in its batch, in a permuted batch, and with outputs pre-filled by 0xFF or 0x00 bytes."""
    heat = torch.from_numpy(planes[0]["p16"]).cuda()
    full = _call(env, heat, fill=0xFF)
    zero = _call(env, heat, fill=0x00)
    for name in OUTS:
        assert _bits(full[name], zero[name]), name
    flat = heat.reshape(9, 1, 16, 16)
    perm = [4, 8, 0, 5, 2, 7, 1, 3, 6]
    shuf = _call(env, flat[perm].reshape(3, 3, 16, 16).contiguous(), fill=0x00)
    for name in OUTS:
        a = full[name].reshape((9,) + full[name].shape[2:])
        b = shuf[name].reshape((9,) + shuf[name].shape[2:])
        assert _bits(a[perm], b), name
    for i in range(9):
        one = _call(env, flat[i:i + 1], fill=0xFF if i % 2 else 0x00)
        for name in OUTS:
            assert _bits(one[name].reshape(-1), full[name].reshape((9, -1))[i]), (name, i)


def test_cov_is_least_squares_pcov(env, planes):
    """On each accepted noisy plane the GPU's deviation from scipy least_squares' cost / (n - 7) (J^T J)^-1 (centre block,
    relative to sqrt(cxx cyy)) is at most 4 x the restatement's own deviation from it, with a floor of 1e-12: the restatement
    differs from the kernel in exp alone, and 4 x is the margin the Gaussian-fit tests give themselves."""
    heat, ref, lsq = planes
    seen = 0
    for key, names in (("p16", NAMES16), ("p40", ["n-wide"])):
        got = _call(env, torch.from_numpy(heat[key]).cuda())
        cov = got["cov"].cpu().numpy().reshape(-1, 3)
        rcov = ref[key][2].reshape(-1, 3)
        for i, name in enumerate(names):
            if lsq[key][i] is None:
                continue
            assert int(got["status"].reshape(-1)[i]) == 0, name
            d_gpu, d_ref = V.deviation(cov[i], lsq[key][i]), V.deviation(rcov[i], lsq[key][i])
            d_rg = V.deviation(cov[i], rcov[i])
            print(f"{name}: GPU - least_squares {d_gpu:.3e}, restatement - least_squares {d_ref:.3e}, GPU - restatement {d_rg:.3e}")
            assert d_gpu <= max(4 * d_ref, 1e-12), (name, d_gpu, d_ref)
            seen += 1
    assert seen == len(V.NOISY)


def test_info_is_the_three_lines_on_the_gpus_own_cov(env, planes):
    """det = cxx cyy - cxy cxy; info = (-(cyy / det), cxy / det, -(cxx / det)) in numpy on the GPU's cov gives the GPU's info bit
    for bit, at the default floor, at 0 and at floors between the cxx and the cyy of fixtures: the floor acts on cxx only."""
    heat = torch.from_numpy(planes[0]["p16"]).cuda()
    base = _call(env, heat)
    cov = base["cov"].cpu().numpy().reshape(9, 3)
    a, b = NAMES16.index("n-border"), NAMES16.index("n-aniso")
    assert cov[a, 0] > cov[a, 2] and cov[b, 0] < cov[b, 2]                   # cxx > cyy in one, cxx < cyy in the other
    fa, fb = 0.5 * (cov[a, 0] + cov[a, 2]), 0.5 * (cov[b, 0] + cov[b, 2])
    for floor in (V.COV_FLOOR, 0.0, fa, fb, 1.0):
        got = _call(env, heat, floor=floor)
        assert _bits(got["cov"], base["cov"]), floor
        want = V.info_of(got["cov"].cpu().numpy(), floor)
        g = got["info"].cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~np.isnan(g)].view(np.int64),
                                                                            want[~np.isnan(want)].view(np.int64)), floor
        info = g.reshape(9, 3)
        if floor == fa:                                                      # cyy < floor <= cxx: kept
            assert np.isfinite(info[a]).all()
        if floor == fb:                                                      # cxx < floor <= cyy: dropped
            assert np.isnan(info[b]).all()
        if floor == 1.0:
            assert np.isnan(info).all()


def test_weights_of_correspondences_mode_1_from_info(env, planes):
    """info in hess_dev's place: w within 4 f64 ulp of the closed form rate (-info)^(1/2) = rate cov^(-1/2), and zero where
    info is NaN; against inv(sqrtm(covar)) of the reference's evaluation.py (scipy) to 1e-10 relative."""
    from scipy.linalg import sqrtm
    inf = env["inference"]
    heat = torch.from_numpy(planes[0]["p16"]).cuda()
    kp, _, _, _, cov, info = inf.gaussfit_keypoints(heat, return_cov=True)
    m, k = 3, 3
    boxes = torch.tensor([[100, 50, 400, 350], [0, 0, 64, 64], [700, 300, 800, 400]], dtype=torch.int32, device="cuda")
    rates = torch.tensor([16 / 300, 0.25, 0.16], dtype=torch.float64, device="cuda")
    valid = torch.ones(m, dtype=torch.int32, device="cuda")
    count, order, pts, w = inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess=info, thresh=-1.0, min_k=k,
                                                            weights="covariance")
    torch.cuda.synchronize()
    hinfo, hcov = info.cpu().numpy(), cov.cpu().numpy()
    ec, eo, _, ew = R.record(kp.cpu().numpy(), boxes.cpu().numpy(), rates.cpu().numpy(), valid.cpu().numpy(), -1.0, k, hinfo)
    assert count.cpu().tolist() == ec.tolist()
    assert order.cpu().tolist() == eo.tolist()
    g = w.cpu().numpy()
    assert np.array_equal(g == 0, ew == 0)
    assert np.all(np.abs(g - ew) <= 4 * np.spacing(np.abs(ew)))
    nz = 0
    for i in range(m):
        for r in range(int(ec[i])):
            j = int(eo[i, r])
            if np.isnan(hinfo[i, j]).any():
                assert (g[i, r] == 0).all(), (i, j)
                continue
            cxx, cxy, cyy = hcov[i, j]
            ref = float(rates[i]) * np.linalg.inv(sqrtm(np.array([[cxx, cxy], [cxy, cyy]])).real)
            assert np.allclose(g[i, r], [ref[0, 0], ref[0, 1], ref[1, 1]], rtol=1e-10, atol=0), (i, j)
            nz += 1
    assert nz == len(ACCEPTED16) - 1                                           # every noisy plane; the clean one is below the floor
    with pytest.raises(ValueError, match="hess"):
        inf.keypoints_to_correspondences(kp, boxes, rates, valid, weights="covariance")


# ---- 2. the fused forms -------------------------------------------------------------------------------------------------------------
FORMS = [("seg_hrnet2", "fp32", "final_gfcov_finish_kernel"),       # VALU output layer re-evaluated into LDS
         ("seg_hrnet2", "bf16x3", "gfcov_kernel"),                   # matrix-core output layer (split bf16): heat-maps in the workspace
         ("seg_hrnet3", "fp32", "gfcov_nhwc_kernel")]                # NHWC heat-maps in the workspace


def _blob_crops(cin):
    """3 crops of 64 x 64: the forward test's blob heat-maps (heat-map k of crop i is a scaled blob_i plus a bias), here with 2 %
    noise on the crop so that the residuals, and with them the covariance, are those of a noisy fit."""
    rng = np.random.default_rng(5)
    x = torch.zeros(3, cin, 64, 64)
    for i, (cx, cy, sx, sy, th) in enumerate([(30.3, 24.6, 2.0, 1.6, 0.7), (3.4, 40.2, 2.0, 2.0, 0.0), (51.7, 60.4, 1.5, 2.5, 0.4)]):
        x[i, 0] = torch.from_numpy((G.blob(64, 64, cx, cy, sx, sy, th)[0] + rng.normal(0.0, 0.02, (64, 64))).astype(np.float32))
    return x


def _raw_forward(env, net, x, ws_fill=None, floor=V.COV_FLOOR, cov=True):
    """esahrnet_forward_keypoints_gaussfit_cov on buffers of the test's own (outputs pre-filled with 0xFF)."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    k = net.num_keypoints
    h = net._rt._handle_for(net, x.device)
    need = C.c_size_t()
    L.check(lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes(h, n, hh, ww, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    o = dict(kp=torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), idx=torch.empty((n, k), dtype=torch.int32, device="cuda"),
             fit=torch.empty((n, k, 8), dtype=torch.float64, device="cuda"), status=torch.empty((n, k), dtype=torch.int32, device="cuda"),
             hess=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"), cov=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"),
             info=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"))
    for t in o.values():
        t.view(torch.uint8).fill_(0xFF)
    L.check(lib.esahrnet_forward_keypoints_gaussfit_cov(h, x.data_ptr(), n, hh, ww, o["kp"].data_ptr(), o["idx"].data_ptr(),
                                                        o["fit"].data_ptr(), o["status"].data_ptr(), o["hess"].data_ptr(),
                                                        o["cov"].data_ptr() if cov else None, o["info"].data_ptr() if cov else None,
                                                        float(floor), wp, need.value,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("name,precision,kernel", FORMS)
def test_fused_forward_equals_forward_plus_the_stand_alone_entry(env, name, precision, kernel):
    """esahrnet_forward_keypoints_gaussfit_cov == esahrnet_forward + esahrnet_keypoints_gaussfit_cov, bit for bit in every
    output, also from a workspace filled with 0xFF and inside a captured graph; without the two pointers it is
    esahrnet_forward_keypoints_gaussfit.  Accepted fits with a finite covariance and a finite info occur."""
    net, _ = F._build(env, name, precision, edit=F._blob_edit(name))
    x = _blob_crops(F.NETS[name][0]).cuda()
    with torch.no_grad():
        heat = net(x)
        want = _call(env, heat)
        got = net.keypoints_gaussfit(x, return_fit=True, return_cov=True)
        old = net.keypoints_gaussfit(x, return_fit=True)
        short = net.keypoints_gaussfit(x, return_cov=True)
    torch.cuda.synchronize()
    ok = want["status"] == 0
    n_cov, n_info = int(torch.isfinite(want["cov"]).all(-1).sum()), int(torch.isfinite(want["info"]).all(-1).sum())
    print(name, precision, kernel, "accepted", int(ok.sum()), "of", ok.numel(), "finite cov", n_cov, "finite info", n_info,
          "median cxx", float(want["cov"][..., 0].nanmedian()))
    assert int(ok.sum()) > 0 and n_cov > 0 and n_info > 0
    assert bool(torch.isnan(want["cov"][~ok]).all()) and bool(torch.isnan(want["info"][~ok]).all())
    for a, nm in zip(got, ("kp", "fit", "status", "hess", "cov", "info")):
        assert _bits(a, want[nm]), nm
    for a, nm in zip(old, ("kp", "fit", "status", "hess")):
        assert _bits(a, want[nm]), nm
    assert len(short) == 5 and _bits(short[3], want["cov"]) and _bits(short[4], want["info"])
    for ws_fill in (None, 0xFF):
        raw = _raw_forward(env, net, x, ws_fill)
        for nm in OUTS:
            assert _bits(raw[nm], want[nm]), (nm, ws_fill)
    raw = _raw_forward(env, net, x, 0xFF, cov=False)
    assert all(_bits(raw[nm], want[nm]) for nm in OUTS[:5]) and _untouched(raw["cov"]) and _untouched(raw["info"])
    zero = _raw_forward(env, net, x, floor=0.0)
    assert _bits(zero["cov"], want["cov"]) and _bits(zero["info"], _call(env, heat, floor=0.0)["info"])
    # inside a captured graph, replayed on another input
    x2 = x.flip(0).contiguous()
    xin = x.clone()
    with torch.no_grad():
        ref2 = [t.clone() for t in net.keypoints_gaussfit(x2, return_fit=True, return_cov=True)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.keypoints_gaussfit(xin, return_fit=True, return_cov=True)
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            out = net.keypoints_gaussfit(xin, return_fit=True, return_cov=True)
        xin.copy_(x2)
        gph.replay()
        torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(out, ref2))
    assert not _bits(ref2[4], want["cov"])


# ---- 3. the loader -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_equals_its_parts(env, name):
    """esahrnet_frames_keypoints_gaussfit_cov: valid rows bit-identical to crops -> esahrnet_forward_keypoints_gaussfit_cov and
    to esahrnet_frames_keypoints_gaussfit; an invalid crop has NaN cov and info; frames_to_correspondences(weights=
    "covariance") equals the loader followed by keypoints_to_correspondences on its info."""
    _loader_equals_its_parts(env, name, "fp32", 64)


def test_loader_equals_its_parts_behind_the_matrix_core_output_layer(env):
    """The same on split bf16, where the output layer is the matrix-core kernel and the fit reads its heat-maps from the
    workspace: the one source of the maps that the loader's Gaussian-fit entries (with and without the covariance, and the
    correspondences behind them) meet in no other test.  Crops of 48 x 48 (the loader's crops are square): partial last tiles
    at every level, and 13 x 13 fit windows that meet the border."""
    _loader_equals_its_parts(env, "seg_hrnet2", "bf16x3", 48)


def _loader_equals_its_parts(env, name, precision, scale):
    inf, crops = env["inference"], env["crops"]
    net, _ = F._build(env, name, precision, gain=1.0)
    frames = F._frames(env, "frames", 2)
    k = net.num_keypoints
    with torch.no_grad():
        x, _, _, _ = crops.crop_batch_device(frames, F.SCENE_BOXES, frame_idx=F.SCENE_FIDX, scale=scale)
        rkp, rfit, rstatus, rhess, rcov, rinfo = net.keypoints_gaussfit(x, return_fit=True, return_cov=True)
        old = net._loader(inf.LoaderRequest("gaussfit"), frames, F.SCENE_BOXES, F.SCENE_FIDX, scale, "val", None, 0.229, None)
        rt = net._rt.frames_keypoints(net, inf.LoaderRequest("gaussfit", None, V.COV_FLOOR), frames, F.SCENE_BOXES, F.SCENE_FIDX, 5,
                                      scale, 0, 0, float(crops.MEAN_VAL), 0.229)
    torch.cuda.synchronize()
    names = ("kp", "boxes", "rates", "valid", "idx", "fit", "status", "hess")
    kp, boxes, rates, valid, idx, fit, status, hess, cov, info = (rt[n] for n in names + ("cov", "info"))
    (packed, _), = rt.records.values()
    assert valid.tolist() == F.SCENE_VALID
    for n in names:
        assert _bits(rt[n], old[n]), n
    good, bad = [i for i, v in enumerate(F.SCENE_VALID) if v], [i for i, v in enumerate(F.SCENE_VALID) if not v]
    assert _bits(kp[good], rkp[good]) and _bits(fit[good], rfit[good]) and torch.equal(status[good], rstatus[good])
    assert _bits(cov[good], rcov[good]) and _bits(info[good], rinfo[good])
    assert bool(torch.isnan(cov[bad]).all()) and bool(torch.isnan(info[bad]).all()) and bool((status[bad] == -1).all())
    assert packed.numel() == inf.packed_layout(5, k, True, cov=True)["total"][1]
    print(name, "statuses -1..3", np.bincount(status.cpu().numpy().ravel() + 1, minlength=5).tolist(), "finite cov",
          int(torch.isfinite(cov).all(-1).sum()), "finite info", int(torch.isfinite(info).all(-1).sum()))
    sel = dict(thresh=0.1, min_k=6)
    with torch.no_grad():
        out = net.frames_to_correspondences(frames, F.SCENE_BOXES, frame_idx=F.SCENE_FIDX, scale=scale, refine="gaussfit",
                                            weights="covariance", **sel)
        parts = inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess=info, weights="covariance", **sel)
    torch.cuda.synchronize()
    assert len(out) == 8 and all(_bits(a, b) for a, b in zip(out[:4], parts))
    assert _bits(out[4], kp) and _bits(out[5], boxes) and _bits(out[6], rates) and _bits(out[7], valid)
    assert [out[0].tolist()[i] for i in bad] == [0, 0]


# ---- 4. the pipeline -------------------------------------------------------------------------------------------------------------------
def test_estimate_poses_with_covariance_weights(env):
    """weights="covariance" runs on the forward test's scene and returns finite poses: the native solver on the record that the
    loader's own outputs give with info in the Hessian's place.  weights="hessian" and weights="peak" give the poses of the
    calls that were there before, bit for bit: esahrnet_frames_keypoints_gaussfit, then esahrnet_correspondences on its own
    hess (mode 1) or without one (mode 0), then the native solver."""
    pipeline, inf, pnp, synth = env["pipeline"], env["inference"], env["pnp"], env["synth"]
    net, _ = F._build(env, "seg_hrnet2", "fp32", gain=1.0)
    n = 6
    scene = synth.make_scene(n, net.num_keypoints, seed=0)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
    sel = dict(thresh=0.0, min_k=8)
    kw = dict(scale=64, on_fail="nan", refine="gaussfit", device_select=True, **sel)
    args = (net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA)
    cam = np.asarray(synth.ESA_CAMERA, np.float64)

    def solve(kp, boxes, rates, valid, hess, weights):
        with torch.no_grad():
            count, order, pts, w = (t.cpu().numpy() for t in inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess=hess,
                                                                                              weights=weights, **sel))
        q, t = pnp.correspondences_to_pose_batch(pts, w, count, order, scene["kp3d"], cam, 0)
        return [(q[i], t[i]) for i in range(n)], w

    got = pipeline.estimate_poses(*args, weights="covariance", **kw)
    assert len(got) == n and all(np.isfinite(q).all() and np.isfinite(t).all() for q, t in got)
    with torch.no_grad():
        rt = net._rt.frames_keypoints(net, inf.LoaderRequest("gaussfit", None, V.COV_FLOOR), frames, scene["bboxes"], None, n, 64, 0, 0,
                                      float(env["crops"].MEAN_VAL), 0.229)
        kp, boxes, rates, valid, status, cov, info = (rt[n_] for n_ in ("kp", "boxes", "rates", "valid", "status", "cov", "info"))
    want, w = solve(kp, boxes, rates, valid, info, "covariance")
    assert F._same_poses(got, want)
    print("statuses 0..3", F._counts(status), "finite info", int(torch.isfinite(info).all(-1).sum()), "points with a weight",
          int((np.abs(w).sum(-1) > 0).sum()))
    with torch.no_grad():
        old = net._loader(inf.LoaderRequest("gaussfit"), frames, scene["bboxes"], None, 64, "val", None, 0.229, None)
        okp, oboxes, orates, ovalid, ohess = (old[n] for n in ("kp", "boxes", "rates", "valid", "hess"))
    assert _bits(okp, kp) and _bits(oboxes, boxes) and _bits(orates, rates)
    for wname, hess in (("peak", None), ("hessian", ohess)):
        assert F._same_poses(pipeline.estimate_poses(*args, weights=wname, **kw), solve(okp, oboxes, orates, ovalid, hess, wname)[0]), wname
