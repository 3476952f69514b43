"""Camera views on the device (rt_scene_view): a view renders, bit for bit, what a scene loaded with
that camera renders, in every kernel family and entry point; it meets the oracle's bar; and a general frame (right
rotated about dir, another fov) traces the rays the definition states."""
import numpy as np
import pytest

import denoise_ref as ref
import reproject_ref as rr
from conftest import scene_path
from test_gpu_parity import _assert_parity

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SCENES = ("cornell_box", "cubes", "flying_unicorn")


@pytest.fixture(scope="module")
def pairs(rt, gpu_scenes, tmp_path_factory):
    """Per scene: (a view of the shared scene with camera A, a scene loaded from the A-camera TOML, that TOML)."""
    out = {}
    tmp = tmp_path_factory.mktemp("moved")
    for name in SCENES:
        va = rr.scene_view(scene_path(name), rr.MOVE_A)
        path, assets = rr.moved_toml(scene_path(name), va, tmp)
        out[name] = (gpu_scenes[name].view(**rr.as_kwargs(va)), rt.Scene.from_toml(path, assets), (path, assets))
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("megakernel", (False, True), ids=("wavefront", "megakernel"))
@pytest.mark.parametrize("name", SCENES)
def test_view_renders_what_the_loaded_scene_renders(rt, pairs, name, megakernel):
    view, loaded, _ = pairs[name]
    got = rt.render(view, 64, 48, 8, SEED, megakernel=megakernel, want_sub=True)
    want = rt.render(loaded, 64, 48, 8, SEED, megakernel=megakernel, want_sub=True)
    assert _same(got[1], want[1]) and _same(got[0], want[0])
    assert got[2]["samples"] == 64 * 48 * 8 and want[1].any()
    base_frame = rt.render(view._base, 64, 48, 8, SEED, megakernel=megakernel, want_sub=True)
    assert not _same(base_frame[1], got[1])  # the camera did move, and the base kept its own


@pytest.mark.parametrize("mode", ("split_tail", "mis", "mis_wavefront", "fp32"))
def test_view_in_the_other_modes_on_cornell(rt, pairs, mode):
    view, loaded, _ = pairs["cornell_box"]
    kw = dict(split_tail=dict(megakernel=True), mis=dict(mis=True, megakernel=True), mis_wavefront=dict(mis=True),
              fp32=dict(fp32=True))[mode]
    w, h, spp = (32, 24, 256) if mode == "split_tail" else (64, 48, 8)
    got = rt.render(view, w, h, spp, SEED, want_sub=True, **kw)
    if mode == "split_tail":
        assert rt.debug_last_split()["split"] > 0
    want = rt.render(loaded, w, h, spp, SEED, want_sub=True, **kw)
    assert _same(got[1], want[1]) and _same(got[0], want[0])


def test_view_in_render_pixels_and_features(rt, pairs):
    for name in ("cornell_box", "flying_unicorn"):
        view, loaded, _ = pairs[name]
        ids = np.sort(np.random.default_rng(3).choice(64 * 48, size=50, replace=False)).astype(np.uint32)
        got = rt.render_pixels(view, 64, 48, ids, 8, SEED, want_sub=True)
        want = rt.render_pixels(loaded, 64, 48, ids, 8, SEED, want_sub=True)
        assert _same(got[1], want[1]) and _same(got[0], want[0])
        full = rt.render(view, 64, 48, 8, SEED, megakernel=True, want_sub=True)[1]
        assert _same(got[1], full.reshape(-1, 4, 3)[ids])
        assert _same(rt.render_features(view, 64, 48), rt.render_features(loaded, 64, 48))


def test_view_queries_and_accumulator_take_the_view(rt, pairs):
    """rt_trace_rays / rt_diag_* answer for the shared geometry; rt_accum_add renders the view's frame."""
    view, loaded, _ = pairs["cubes"]
    o, d = rr.centre_rays(rr.scene_view(scene_path("cubes"), rr.MOVE_A), 16, 12)
    for a, b in zip(view.trace_ray(o, d), loaded.trace_ray(o, d)):
        assert _same(a, b)
    for a, b in zip(view.diag_trace(o, d), view._base.diag_trace(o, d)):
        assert _same(a, b)
    with rt.Accumulator(32, 24) as acc:
        acc.add(view, 8, SEED)
        sub = acc.resolve()[0]
    assert _same(sub, rt.render(loaded, 32, 24, 8, SEED, megakernel=True, want_sub=True)[1])


@pytest.mark.parametrize("name", ("cornell_box", "cubes"))
def test_view_against_the_oracle(rt, oracle, pairs, name):
    view, _, (path, assets) = pairs[name]
    osc = oracle.OracleScene(path, assets_dir=assets)
    w, h, spp = 48, 36, 8
    rgb_o, sub_o, _ = osc.render(w, h, spp, SEED)
    for mk in (False, True):
        rgb, sub, _ = rt.render(view, w, h, spp, SEED, megakernel=mk, want_sub=True)
        _assert_parity(rgb, sub, rgb_o, sub_o, f"{name} view, megakernel={mk}")


@pytest.mark.parametrize("name", ("cornell_box", "flying_unicorn"))
def test_general_frame_traces_the_stated_rays(rt, gpu_scenes, oracle_scenes, name):
    """right rotated 25 degrees about dir (and not unit length), fov = 0.8: rt_render_features' depth and normal
    against the oracle's trace of the numpy-built centre rays at 1e-6, with test_gpu_features.py's exclusion rule
    (pixels whose hit objects differ between rt_trace_rays of the same rays and the oracle) and its 0.1 % cap."""
    w, h = 96, 72
    v0 = rr.scene_view(scene_path(name), rr.MOVE_A)
    d = v0["dir"] / np.sqrt(v0["dir"].dot(v0["dir"]))
    r0 = np.cross(d, np.array([0.0, 1.0, 0.0]))
    r0 /= np.sqrt(r0.dot(r0))
    ang = np.deg2rad(25.0)
    right = (r0 * np.cos(ang) + np.cross(d, r0) * np.sin(ang)) * 1.25
    v = rr.view(v0["pos"], v0["dir"], right, 0.8)
    scene = gpu_scenes[name].view(**rr.as_kwargs(v))
    assert scene.camera() == rr.as_kwargs(v)
    feat = rt.render_features(scene, w, h)
    o, dirs = rr.centre_rays(v, w, h)
    t, ids, _, nrm = ref.trace_parallel(oracle_scenes[name], o, dirs)
    n_ref, z_ref, k_ref, ids = ref.features_from_hits(t, ids, nrm, w, h)
    _, ids_dev, _, _ = scene.trace_ray(o, dirs)
    same = (ids_dev.reshape(h, w, 4) == ids).all(-1)
    excluded = int((~same).sum())
    print(f"{name}: {excluded} pixels excluded, coverage mean {k_ref.mean():.3f}")
    assert excluded <= 6  # 0.1 % of 6,912 pixels
    f = feat.astype(np.float64)
    close = lambda a, b: np.abs(a - b) <= 1e-6 * np.abs(b) + 1e-37
    assert np.array_equal(feat[..., 7][same], k_ref[same].astype(np.float32)) and (k_ref > 0).mean() > 0.5
    assert close(f[..., 0:3][same], n_ref[same]).all()
    assert close(f[..., 3][same], z_ref[same]).all()
    # and it is not the reference frame's image: the rotated frame sees other objects somewhere
    plain = rt.render_features(gpu_scenes[name].view(**rr.as_kwargs(v0)), w, h)
    assert not np.array_equal(plain, feat)
