"""Camera views (rt_scene_view, rt_scene_get_view) without a GPU: the argument checks, the round trip,
the sharing rules, the Python, ctypes and Rust mirrors, and the server's camera message."""
import asyncio
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path

NAMES = ["rt_scene_view", "rt_scene_get_view", "rt_accum_reproject"]
RT_E_INVAL = -1

OBJS = [dict(geom_kind=1, pos=[0.0, 0.0, 0.0], n=[0.0, 1.0, 0.0], brdf_kind=0, k=[0.5, 0.5, 0.5]),
        dict(geom_kind=0, pos=[0.0, 5.0, 0.0], r=1.0, brdf_kind=0, k=[0.0, 0.0, 0.0], emitted=[10.0, 10.0, 10.0])]


@pytest.fixture(scope="module")
def scene(rt):
    return rt.Scene.from_desc([0.0, 2.0, 10.0], [0.0, -0.1, -1.0], OBJS)


def _view(rt, pos, d, right=(1.0, 0.0, 0.0), fov=0.5135):
    v = rt.View()
    for j in range(3):
        v.pos[j], v.dir[j], v.right[j] = pos[j], d[j], right[j]
    v.fov = fov
    return v


def test_declared_in_every_mirror(rt):
    header = open(os.path.join(REPO, "include", "rt_ffi.h")).read()
    rust = open(os.path.join(REPO, "ffi", "raytracer_ffi.rs")).read()
    for n in NAMES:
        assert hasattr(rt.lib, n), f"missing export {n}"
        assert re.search(rf"^int {n}\(", header, re.M), f"{n} not declared in rt_ffi.h"
        assert re.search(rf"pub fn {n}\s*\(", rust), f"{n} not declared in raytracer_ffi.rs"
        assert n in rt._EXPORTS
        assert getattr(rt.lib, n).argtypes is not None
    assert re.search(r"typedef struct \{ double pos\[3\], dir\[3\], right\[3\]; double fov; \} rt_view;", header)
    assert "pub type RtView = [f64; 10];" in rust
    assert ctypes.sizeof(rt.View) == 80 and [f[0] for f in rt.View._fields_] == ["pos", "dir", "right", "fov"]
    assert rt.lib.rt_abi_version() == 3  # additive
    for f in ("look_at", "render_interactive"):
        assert callable(getattr(rt, f))
    for m in ("view", "camera"):
        assert callable(getattr(rt.Scene, m))
    assert callable(rt.Accumulator.reproject_from)
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(n in text for n in NAMES)


def test_loaded_scene_reports_the_reference_camera(rt, scene):
    c = scene.camera()
    assert c == dict(pos=(0.0, 2.0, 10.0), dir=(0.0, -0.1, -1.0), right=(1.0, 0.0, 0.0), fov=0.5135)
    s = rt.Scene.from_toml(scene_path("cornell_box"))
    assert s.camera() == dict(pos=(50.0, 52.0, 295.6), dir=(0.0, -0.042612, -1.0), right=(1.0, 0.0, 0.0), fov=0.5135)


def test_view_round_trips(rt, scene):
    kw = dict(pos=(1.5, -2.25, 1e6), dir=(0.3, 0.1, -0.9), right=(0.8, 0.0, 0.6), fov=0.8)
    v = scene.view(**kw)
    assert v.camera() == kw
    assert scene.camera()["pos"] == (0.0, 2.0, 10.0)  # the base keeps its own camera
    assert scene.view((1.0, 2.0, 3.0), (0.0, 0.0, -1.0)).camera()["right"] == (1.0, 0.0, 0.0)


def test_view_of_a_view_refers_to_the_root(rt):
    base = rt.Scene.from_toml(scene_path("cubes"))
    v1 = base.view((0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
    v2 = v1.view((5.0, 0.0, 1.0), (0.0, 0.1, -1.0), fov=0.7)
    assert v2._base is base and v1._base is base
    assert v2.info() == base.info() == v1.info() and base.info()["meshes"] > 0
    m = [o for o in range(base.info()["objects"]) if _is_mesh(base, o)][0]
    assert np.array_equal(v2.mesh(m)["vertices"], base.mesh(m)["vertices"])
    v1.close()  # releasing the middle view touches nothing shared
    assert v2.info() == base.info() and v2.camera()["fov"] == 0.7
    v2.close()
    assert base.info()["meshes"] > 0


def _is_mesh(scene, obj):
    try:
        scene.mesh(obj)
        return True
    except Exception:
        return False


BAD = {
    "nan pos": dict(pos=(math.nan, 0.0, 0.0)),
    "inf pos": dict(pos=(0.0, math.inf, 0.0)),
    "nan dir": dict(d=(0.0, math.nan, -1.0)),
    "inf dir": dict(d=(0.0, 0.0, -math.inf)),
    "nan right": dict(right=(math.nan, 0.0, 0.0)),
    "inf right": dict(right=(math.inf, 0.0, 0.0)),
    "nan fov": dict(fov=math.nan),
    "inf fov": dict(fov=math.inf),
    "zero fov": dict(fov=0.0),
    "negative fov": dict(fov=-0.5),
    "right parallel to dir": dict(d=(0.0, 0.0, -1.0), right=(0.0, 0.0, 2.0)),
    "zero right": dict(right=(0.0, 0.0, 0.0)),
    "zero dir": dict(d=(0.0, 0.0, 0.0)),
    "cross overflows": dict(d=(0.0, 1e200, 0.0), right=(1e200, 0.0, 0.0)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_views_are_invalid(rt, scene, case):
    a = dict(pos=(0.0, 0.0, 0.0), d=(0.0, 0.0, -1.0), right=(1.0, 0.0, 0.0), fov=0.5135)
    a.update(BAD[case])
    h = ctypes.c_void_p(1234)
    rc = rt.lib.rt_scene_view(scene.handle, ctypes.byref(_view(rt, a["pos"], a["d"], a["right"], a["fov"])),
                              ctypes.byref(h))
    assert rc == RT_E_INVAL and not h.value, case
    assert b"rt_scene_view" in rt.lib.rt_last_error()


def test_null_arguments_are_invalid(rt, scene):
    good = _view(rt, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    h = ctypes.c_void_p()
    assert rt.lib.rt_scene_view(None, ctypes.byref(good), ctypes.byref(h)) == RT_E_INVAL
    assert rt.lib.rt_scene_view(scene.handle, None, ctypes.byref(h)) == RT_E_INVAL
    assert rt.lib.rt_scene_view(scene.handle, ctypes.byref(good), None) == RT_E_INVAL
    assert rt.lib.rt_scene_get_view(None, ctypes.byref(good)) == RT_E_INVAL
    assert rt.lib.rt_scene_get_view(scene.handle, None) == RT_E_INVAL
    with pytest.raises(rt.RtError):
        scene.view((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=0.0)


def test_look_at(rt):
    v = rt.look_at((50.0, 52.0, 295.6), (50.0, 52.0, 0.0))
    assert v["dir"] == (0.0, 0.0, -1.0) and v["right"] == (1.0, 0.0, 0.0) and v["fov"] == 0.5135
    v = rt.look_at((1.0, 2.0, 3.0), (4.0, 0.0, -2.0), up=(0.0, 1.0, 0.0), fov=0.7)
    d, r = np.array(v["dir"]), np.array(v["right"])
    assert abs(d.dot(d) - 1.0) < 1e-15 and abs(r.dot(r) - 1.0) < 1e-15 and abs(d.dot(r)) < 1e-15
    assert abs(r[1]) < 1e-15 and v["pos"] == (1.0, 2.0, 3.0) and v["fov"] == 0.7
    want = np.array([3.0, -2.0, -5.0])
    assert np.allclose(d, want / np.linalg.norm(want), rtol=0, atol=1e-15)


# The server's camera message ---------------------------------------------------------------------------------

def test_parse_camera():
    from rt_amd import server

    assert server.parse_camera({"type": "render"}) is None
    assert server.parse_camera({"camera": {"pos": [1, 2, 3], "dir": [0, 0, -1]}}) == \
        dict(pos=(1.0, 2.0, 3.0), dir=(0.0, 0.0, -1.0))
    assert server.parse_camera({"camera": {"pos": [1, 2, 3], "dir": [0, 0, -1], "right": [1, 0, 0], "fov": 1}}) == \
        dict(pos=(1.0, 2.0, 3.0), dir=(0.0, 0.0, -1.0), right=(1.0, 0.0, 0.0), fov=1.0)
    for bad in ([1, 2, 3], {"pos": [1, 2, 3]}, {"dir": [0, 0, -1]}, {"pos": [1, 2], "dir": [0, 0, -1]},
                {"pos": [1, 2, "3"], "dir": [0, 0, -1]}, {"pos": [1, 2, 3], "dir": [0, 0, -1], "fov": "wide"},
                {"pos": [1, 2, 3], "dir": [0, 0, -1], "up": [0, 1, 0]}, {"pos": [1, 2, True], "dir": [0, 0, -1]},
                {"pos": "here", "dir": [0, 0, -1]}):
        with pytest.raises(ValueError):
            server.parse_camera({"camera": bad})


class _FakeScene:
    def __init__(self, cam=None):
        self.cam = cam

    def view(self, **kw):
        if kw.get("fov", 1.0) <= 0:
            raise RuntimeError("rt error -1: fov must be > 0")
        return _FakeScene(kw)


class _FakeJob:
    """RenderJob's interface; records the scene each request was run with."""

    def __init__(self, seen):
        self.seen = seen
        self.busy = False

    def running(self):
        return self.busy

    def stop(self):
        pass

    async def run(self, scene, width, height, spp, seed):
        self.seen.append((scene.cam, spp))
        return False


def test_server_hands_the_view_to_the_job():
    from aiohttp import ClientSession, web
    from rt_amd import server

    seen, logs = [], []
    srv = server.Server({"cornell_box": _FakeScene()}, width=8, height=6, log=logs.append,
                        job_factory=lambda send: _FakeJob(seen))
    req = {"type": "render", "scene": "cornell_box", "spp": 8}
    cam = {"pos": [1, 2, 3], "dir": [0, 0.5, -1], "fov": 0.75}
    msgs = [dict(req), dict(req, camera=cam), dict(req, camera={"pos": [1, 2, 3]}),
            dict(req, camera=dict(cam, fov=0)), dict(req, spp=12, camera=dict(cam, right=[0, 0, 1]))]

    async def session():
        runner = web.AppRunner(srv.app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        port = site._server.sockets[0].getsockname()[1]
        try:
            async with ClientSession() as cs:
                async with cs.ws_connect(f"http://127.0.0.1:{port}/") as ws:
                    for m in msgs:
                        await ws.send_str(json.dumps(m))
                    await ws.close()
        finally:
            await runner.cleanup()

    asyncio.run(session())
    assert seen == [(None, 8), (dict(pos=(1.0, 2.0, 3.0), dir=(0.0, 0.5, -1.0), fov=0.75), 8),
                    (dict(pos=(1.0, 2.0, 3.0), dir=(0.0, 0.5, -1.0), fov=0.75, right=(0.0, 0.0, 1.0)), 12)]
    bad = [ln for ln in logs if "bad render request" in ln]
    assert len(bad) == 2  # the camera without dir and the one the scene refused, each logged, the connection kept
