"""First-hit feature buffers (rt_render_features, k_features_f64) against the CPU oracle's trace of the same
centre rays, the albedo definition, and the tile mapping."""
import numpy as np
import pytest

import denoise_ref as ref
from conftest import scene_path

pytestmark = pytest.mark.gpu

W, H = 96, 72
CASES = (("cornell_box", False), ("cubes", False), ("flying_unicorn", False), ("flying_unicorn", True))
MAX_EXCLUDED = 6  # 0.1 % of 6,912 pixels


def _close(a, b, rel=1e-6):
    """1e-6 relative (f32 rounding plus the reduction order); 1e-37: below it f32 is subnormal."""
    return np.abs(a - b) <= rel * np.abs(b) + 1e-37


@pytest.mark.parametrize("name,nearest", CASES)
def test_features_match_oracle_trace(rt, gpu_scenes, oracle, oracle_scenes, name, nearest):
    """Normal, depth and coverage of every pixel whose four centre rays hit the same objects on the device
    (rt_trace_rays of the same rays) and in the oracle agree to 1e-6 relative; at most 6 of 6,912 pixels may differ
    in a hit object and are excluded. On the CPU the oracle alone changes the hit objects of 0 pixels in each of the
    four cases when every direction component moves one ulp
    (tests/test_denoise_abi.py::test_oracle_hit_objects_stable_under_one_ulp)."""
    feat = rt.render_features(gpu_scenes[name], W, H, mesh_nearest=nearest)
    assert feat.shape == (H, W, 8) and feat.dtype == np.float32 and np.isfinite(feat).all()
    osc = oracle.OracleScene(scene_path(name), mesh_nearest=True) if nearest else oracle_scenes[name]
    o, d = ref.centre_rays(*ref.camera_of(scene_path(name)), W, H)
    t, ids, _, nrm = ref.trace_parallel(osc, o, d)
    n_ref, z_ref, k_ref, ids = ref.features_from_hits(t, ids, nrm, W, H)
    _, ids_dev, _, _ = gpu_scenes[name].trace_ray(o, d, mesh_nearest=nearest)
    same = (ids_dev.reshape(H, W, 4) == ids).all(-1)
    excluded = int((~same).sum())
    print(f"{name} nearest={nearest}: {excluded} pixels excluded, coverage mean {k_ref.mean():.3f}")
    assert excluded <= MAX_EXCLUDED
    assert np.array_equal(feat[..., 7] * 4, np.round(feat[..., 7] * 4))  # an exact multiple of 0.25
    assert np.array_equal(feat[..., 7][same], k_ref[same].astype(np.float32))
    assert (k_ref > 0).mean() > 0.5
    f = feat.astype(np.float64)
    assert _close(f[..., 0:3][same], n_ref[same]).all()
    assert _close(f[..., 3][same], z_ref[same]).all()
    miss = same & (k_ref == 0)
    assert not f[miss].any()  # every mean is 0 where no ray hit


def test_albedo_definition(rt):
    """clamp(base + emitted, 0, 1): base = k for diffuse and specular, phong_kd * color_d + phong_ks * color_s for
    Phong. Four spheres; interior pixels (all four centre rays on one object) against the definition to 1e-6."""
    w, h = 64, 48
    objs = [
        dict(geom_kind=0, pos=[-1.7, 1.3, 0], r=1.0, brdf_kind=0, k=[0.2, 0.4, 0.6]),
        dict(geom_kind=0, pos=[1.7, 1.3, 0], r=1.0, brdf_kind=1, k=[0.9, 0.8, 0.7]),
        dict(geom_kind=0, pos=[-1.7, -1.3, 0], r=1.0, brdf_kind=2, phong_kd=0.6, phong_ks=0.3, phong_power=10,
             color_d=[0.5, 0.25, 1.0], color_s=[1.0, 1.0, 0.5]),
        dict(geom_kind=0, pos=[1.7, -1.3, 0], r=1.0, brdf_kind=0, k=[0.1, 0.1, 0.1], emitted=[0.5, 2.0, 0.0]),
    ]
    want = np.array([[0.2, 0.4, 0.6], [0.9, 0.8, 0.7],
                     [0.6 * 0.5 + 0.3 * 1.0, 0.6 * 0.25 + 0.3 * 1.0, 0.6 * 1.0 + 0.3 * 0.5], [0.6, 1.0, 0.1]])
    want = np.clip(want, 0.0, 1.0)
    cam_pos, cam_dir = [0.0, 0.0, 10.0], [0.0, 0.0, -1.0]
    scene = rt.Scene.from_desc(cam_pos, cam_dir, objs)
    feat = rt.render_features(scene, w, h)
    o, d = ref.centre_rays(np.array(cam_pos), np.array(cam_dir), w, h)
    _, ids, _, _ = scene.trace_ray(o, d)
    ids = ids.reshape(h, w, 4)
    for k in range(4):
        inside = (ids == k).all(-1)
        assert inside.sum() >= 9, (k, int(inside.sum()))
        assert np.abs(feat[inside][:, 4:7] - want[k]).max() <= 1e-6
        assert (feat[inside][:, 7] == 1.0).all()
    empty = (ids < 0).all(-1)
    assert empty.sum() > 100 and not feat[empty].any()


@pytest.mark.parametrize("name", ("cornell_box", "flying_unicorn"))
def test_tiles_are_crops_of_the_frame(rt, gpu_scenes, name):
    """x0, y0, tile_w, tile_h and row_step map like rt_render's: a tile is the crop of the full frame, bit for bit."""
    full = rt.render_features(gpu_scenes[name], W, H)
    tile = rt.render_features(gpu_scenes[name], W, H, tile=(13, 7, 41, 29))
    assert np.array_equal(tile.view(np.uint32), full[7:36, 13:54].view(np.uint32))
    rows = rt.render_features(gpu_scenes[name], W, H, tile=(5, 2, 50, 20), row_step=3)
    assert np.array_equal(rows.view(np.uint32), full[2:62:3, 5:55].view(np.uint32))
    assert full[..., 7].max() == 1.0
