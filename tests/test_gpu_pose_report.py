"""The pose report behind the device path (pnp.PoseReport, pipeline.estimate_poses(return_report=True)): on the device-select
pipeline it changes no pose and equals the report of the native solver on the fetched correspondence record, for each decoder
and weighting; on rendered heat-maps of a known pose its rms reprojection error is the one the returned pose has."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 32, 64)
BOXES = [(10, 8, 90, 80), (30, 20, 120, 90), (4, 6, 100, 70), (50, 50, 50, 50)]          # position 3: an empty box
FIDX = [0, 1, 1, 2]                                                                       # two boxes on frame 1
SEL = dict(thresh=0.0, min_k=8)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import config, inference, pipeline, pnp, seg_hrnet2, synth
    net = seg_hrnet2.get_seg_model(config.make_config(widths=WIDTHS))
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=53, gain=1.0), strict=True)
    net = net.cuda().eval()
    assert net.num_keypoints == 11
    frames = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(3, 96, 128), dtype=np.uint8)).cuda()
    return dict(net=net, frames=frames, inference=inference, pipeline=pipeline, pnp=pnp, synth=synth,
                kp3d=synth.make_scene(1, 11, seed=0)["kp3d"], K=np.asarray(synth.ESA_CAMERA, np.float64))


def _same_poses(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1], equal_nan=True)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("refine,weights", [("get_final", "peak"), ("get_final2", "hessian"), ("gaussfit", "covariance")])
def test_device_select_pipeline_reports(env, refine, weights):
    net, pipeline, pnp = env["net"], env["pipeline"], env["pnp"]
    args = (net, env["frames"], BOXES, env["kp3d"], env["K"])
    kw = dict(scale=64, frame_idx=FIDX, device_select=True, on_fail="nan", refine=refine, weights=weights, threads=4, **SEL)
    plain = pipeline.estimate_poses(*args, **kw)
    poses, rep = pipeline.estimate_poses(*args, return_report=True, **kw)
    assert _same_poses(poses, plain)
    with torch.no_grad():
        count, order, pts, w = (t.cpu().numpy() for t in net.frames_to_correspondences(
            env["frames"], BOXES, frame_idx=FIDX, scale=64, refine=refine, weights=weights, **SEL)[:4])
    q, t, want = pnp.correspondences_to_pose_batch(pts, w, count, order, env["kp3d"], env["K"], 1, report=True)
    assert rep.raw.tobytes() == want.raw.tobytes()
    assert _same_poses(poses, [(q[i], t[i]) for i in range(4)])
    assert count.tolist()[3] == 0 and (rep.status[3], rep.n[3]) == (1, 0) and np.isnan(np.delete(rep.raw[3], [0, 2])).all()
    assert np.isnan(poses[3][0]).all() and not rep.gated.any()
    assert (rep.n[:3] >= 8).all() and set(rep.status[:3].tolist()) <= {0, 2}
    print(refine, weights, "status", rep.status.tolist(), "n", rep.n.tolist(), "inliers", rep.inliers.tolist(), "rms_px",
          np.round(rep.rms_px, 2).tolist())


def test_report_on_rendered_heatmaps(env):
    """Two images of sigma-2 blobs at the projections of known poses -> get_final2 with its Hessian -> device correspondences
    -> the native solve: every keypoint is an inlier, and rms_px is the rms distance between the record's points and the
    projections under the returned (q, t), to relative 1e-9."""
    inference, pnp, synth = env["inference"], env["pnp"], env["synth"]
    m, k, size = 2, 11, 64
    scene = synth.make_scene(m, k, seed=3)
    uv = scene["uv"]
    lo, hi = uv.min(1), uv.max(1)
    side = np.ceil((hi - lo).max(1) * 1.25 + 8)                                    # a square crop box with a margin
    origin = np.floor((lo + hi) / 2 - side[:, None] / 2)
    rates = size / side
    centers = (uv - origin[:, None, :]) * rates[:, None, None]
    assert centers.min() > 4 and centers.max() < size - 5
    heat = synth.render_heatmaps(torch.from_numpy(centers).float().cuda(), size, 2.0)
    assert tuple(heat.shape) == (m, k, size, size)
    boxes = torch.from_numpy(np.concatenate([origin, origin + side[:, None]], 1).astype(np.int32)).cuda()
    with torch.no_grad():
        kp, hess = inference.heatmaps_to_keypoints(heat, refine="get_final2", return_hessian=True)
        rec = inference.keypoints_to_correspondences(kp, boxes, torch.from_numpy(rates).cuda(), torch.ones(m, dtype=torch.int32).cuda(),
                                                     hess=hess, thresh=0.5, min_k=k, weights="hessian")
    count, order, pts, w = (t.cpu().numpy() for t in rec)
    q, t, rep = pnp.correspondences_to_pose_batch(pts, w, count, order, scene["kp3d"], env["K"], 2, report=True)
    assert rep.status.tolist() == [0, 0] and rep.inliers.tolist() == [k, k] and rep.n.tolist() == [k, k] and (rep.flags == 0).all()
    for i in range(m):
        d = pnp.project(scene["kp3d"][order[i]], pnp.quat_wxyz_to_rotation(q[i]), t[i], env["K"]) - pts[i]
        rms = np.sqrt(np.mean(np.sum(d * d, 1)))
        print(f"image {i}: rms_px {rep.rms_px[i]:.6f} recomputed {rms:.6f}, relative difference {abs(rep.rms_px[i] - rms) / rms:.2e}")
        assert abs(rep.rms_px[i] - rms) <= 1e-9 * rms
        assert rep.min_depth[i] > 0
        print("   SPEED score against the rendered pose", pnp.speed_score(q[i], t[i], scene["q"][i], scene["t"][i])[0])
    assert np.isfinite(rep.covariance()).all()
