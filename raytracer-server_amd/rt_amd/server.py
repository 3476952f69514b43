"""WebSocket front-end on the C ABI: the reference's server.rs protocol, rendering on the GPU.

Mirrors src/server.rs of SuneelFreimuth/raytracer-server:
  * connection ids: 5 distinct lowercase letters (server.rs:63-78);
  * client messages (server.rs:121-126): {"type": "render", "scene": <name>, "spp": <int>} starts a
    job when none is running; {"type": "stop_rendering"} cancels the running job;
  * server messages (server.rs:173-190): binary [u8 type = 0][u8 n][u16le x][u16le y][n x RGB8],
    one per 60-pixel window of a screen row (row 0 = top);
  * frame size 600 x 450 (server.rs:29-30), spp semantics of sample_pixel (4*floor(spp/4) traced).
Differences, by design: the render runs on the GPU through rt_render in row bands (progressive
streaming, band by band, top to bottom), the cancel flag is also polled inside the render, and the
reference's panics (bad JSON, unknown scene) become logged errors.

Run:  PORT=8080 python -m rt_amd.server <scenes dir>
      RT_DENOISE=<levels> selects denoised previews (whole frames through rt_amd.render_denoised).
      RT_PROGRESSIVE=<first_spp> selects progressive jobs (whole frames through rt_amd.render_progressive, each refined
      frame re-sent with the same chunk messages).
      RT_TARGET_ERROR=<abs_tol> selects jobs rendered to a per-pixel error target (rt_amd.render_to_error, DESIGN.md
      §13): RT_PROGRESSIVE gives the first frame's spp, the request's spp is the per-pixel budget.
      RT_TARGET_BATCH=<C>[,<gain>] together with RT_TARGET_ERROR: up to <C> (1..16) sparse passes per pixel run in one
      launch, each batch handing out <gain> (in (0, 1]; default: rt_amd.ERROR_TARGET_BATCH_DEFAULTS) of a pixel's
      predicted need (rt_amd.render_to_error's batch and gain; a mesh scene's batches run its own pool
      kernel, §18). Unset: the sequential loop.
      RT_REPROJECT=<max_n> together with RT_PROGRESSIVE or RT_TARGET_ERROR: a connection keeps its last accumulator
      and view, and a request for the same scene starts from the reprojected history (rt_amd.render_interactive,
      DESIGN.md §14; at most max_n samples per subpixel are inherited).
      RT_REPROJECT_FILL=<spp>[,<refresh>] together with RT_REPROJECT: from a connection's second request on, the two
      full-frame passes are replaced by two sparse passes of <spp> over the pixels that received no history, and every
      pixel gets one fresh pass once in <refresh> requests (0, the default: never). Unset: unchanged.
Beyond the reference's protocol the render message takes an optional camera, {"type": "render", ..., "camera":
{"pos": [x, y, z], "dir": [x, y, z], "right": [x, y, z] (optional), "fov": f (optional)}}: the scene is rendered
through Scene.view of it. Without it nothing changes; a bad camera is a logged error, like a bad scene name.
"""
import asyncio
import ctypes
import json
import os
import random
import string
import struct
import sys

import numpy as np

WIDTH = 600   # server.rs:29
HEIGHT = 450  # server.rs:30
PIXELS_PER_MSG = 60  # server.rs:145
SCENE_NAMES = ("cornell_box", "cubes", "flying_unicorn")  # main.rs:17


def chunk_messages(rgb, y0):
    """Binary messages for rows y0.. of a rendered band (server.rs:173-190)."""
    rows, width, _ = rgb.shape
    for r in range(rows):
        for x in range(0, width, PIXELS_PER_MSG):
            n = min(PIXELS_PER_MSG, width - x)
            yield struct.pack("<BBHH", 0, n, x, y0 + r) + rgb[r, x:x + n].tobytes()


def parse_camera(m):
    """The render message's optional "camera" as Scene.view's keyword arguments, or None without one. ValueError for
    anything but {"pos": 3 numbers, "dir": 3 numbers[, "right": 3 numbers][, "fov": number]}."""
    cam = m.get("camera")
    if cam is None:
        return None

    def num(x):
        return isinstance(x, (int, float)) and not isinstance(x, bool)

    if not isinstance(cam, dict) or set(cam) - {"pos", "dir", "right", "fov"} or "pos" not in cam or "dir" not in cam:
        raise ValueError(f"bad camera {cam!r}")
    out = {}
    for key in ("pos", "dir", "right"):
        if key in cam:
            v = cam[key]
            if not isinstance(v, list) or len(v) != 3 or not all(num(x) for x in v):
                raise ValueError(f"bad camera {key} {v!r}")
            out[key] = tuple(float(x) for x in v)
    if "fov" in cam:
        if not num(cam["fov"]):
            raise ValueError(f"bad camera fov {cam['fov']!r}")
        out["fov"] = float(cam["fov"])
    return out


def parse_fill(text):
    """RT_REPROJECT_FILL's value "<spp>[,<refresh>]" as (fill_spp, refresh); (0, 0) for None (unset: no fill).
    ValueError for anything but one or two integers with spp >= 4 and refresh >= 0."""
    if text is None:
        return 0, 0
    parts = text.split(",")
    if len(parts) not in (1, 2):
        raise ValueError(f"bad RT_REPROJECT_FILL {text!r}")
    spp, refresh = int(parts[0]), int(parts[1]) if len(parts) == 2 else 0
    if spp < 4 or refresh < 0:
        raise ValueError(f"bad RT_REPROJECT_FILL {text!r}: spp must be >= 4 and refresh >= 0")
    return spp, refresh


def parse_batch(text):
    """RT_TARGET_BATCH's value "<C>[,<gain>]" as (batch, gain); (0, None) for None (unset: the sequential loop), gain
    None when only C is given. ValueError for anything but an integer C in 1 .. 16 and a gain in (0, 1]."""
    if text is None:
        return 0, None
    parts = text.split(",")
    if len(parts) not in (1, 2):
        raise ValueError(f"bad RT_TARGET_BATCH {text!r}")
    batch = int(parts[0])
    gain = float(parts[1]) if len(parts) == 2 else None
    if batch < 1 or batch > 16 or (gain is not None and not 0.0 < gain <= 1.0):
        raise ValueError(f"bad RT_TARGET_BATCH {text!r}: C must be in 1 .. 16 and gain in (0, 1]")
    return batch, gain


def gpu_band_renderer(device=0, fp32=False):
    """Default band renderer: rt_render on `device` for rows [y0, y0 + rows). fp32: the f32 perf mode
    (RT_FLAG_FP32, statistical parity only) — server-wide, the protocol is unchanged."""
    import rt_amd

    def render(scene, width, height, spp, seed, y0, rows, cancel):
        rgb, _, st = rt_amd.render(scene, width, height, spp, seed, tile=(0, y0, width, rows),
                                   megakernel=True, device=device, cancel=cancel, fp32=fp32)
        return None if st["cancelled"] else rgb

    return render


def gpu_denoised_frame_renderer(device=0, **denoise_params):
    """Whole-frame renderer with a denoised preview (rt_amd.render_denoised: render + feature buffers + the a-trous
    filter), for a server run with band_rows = height: the filter at a row reads rows up to
    2 * (2^levels - 1) away, so it renders, filters the whole frame and returns the rows it is asked for.
    denoise_params: levels / sigma_* (rt_amd.DENOISE_DEFAULTS otherwise)."""
    import rt_amd

    def render(scene, width, height, spp, seed, y0, rows, cancel):
        rgb = rt_amd.render_denoised(scene, width, height, spp, seed, device=device, cancel=cancel, **denoise_params)
        return None if rgb is None else rgb[y0:y0 + rows]

    return render


class RenderJob:
    """server.rs:139-223: one job per connection, cancellable between bands."""

    def __init__(self, send, renderer, band_rows):
        self.send = send
        self.renderer = renderer
        self.band_rows = band_rows
        self.cancel = ctypes.c_int32(1)  # starts cancelled == not running (server.rs:148-149)

    def running(self):
        return self.cancel.value == 0

    def stop(self):
        self.cancel.value = 1

    async def run(self, scene, width, height, spp, seed):
        """Returns True when stopped before completion (server.rs:156)."""
        self.cancel.value = 0
        loop = asyncio.get_running_loop()
        for y0 in range(0, height, self.band_rows):
            if self.cancel.value:
                return True
            rows = min(self.band_rows, height - y0)
            rgb = await loop.run_in_executor(None, self.renderer, scene, width, height, spp, seed, y0, rows,
                                             self.cancel)
            if rgb is None or self.cancel.value:
                return True
            for msg in chunk_messages(rgb, y0):
                try:
                    await self.send(msg)
                except ConnectionError:
                    self.cancel.value = 1
                    return True
        self.cancel.value = 1
        return False


class ProgressiveJob:
    """A whole-frame job that refines its frame pass by pass (rt_amd.render_progressive): every
    refined frame is sent again with the same chunk messages (they carry x and y, so a client simply overwrites).
    RenderJob's interface: a stop takes effect between passes, and inside a pass through the cancel word."""

    def __init__(self, send, first=8, device=0, **denoise_params):
        self.send = send
        self.first = first
        self.device = device
        self.denoise_params = denoise_params
        self.cancel = ctypes.c_int32(1)  # starts cancelled == not running

    def running(self):
        return self.cancel.value == 0

    def stop(self):
        self.cancel.value = 1

    async def run(self, scene, width, height, spp, seed):
        """Returns True when stopped before the last frame was sent."""
        import rt_amd

        self.cancel.value = 0
        loop = asyncio.get_running_loop()
        frames = rt_amd.render_progressive(scene, width, height, spp, first=self.first, seed=seed, device=self.device,
                                           cancel=self.cancel, **self.denoise_params)
        total = 4 * (spp // 4)
        try:
            while True:
                if self.cancel.value:
                    return True
                frame = await loop.run_in_executor(None, next, frames, None)
                if frame is None or self.cancel.value:
                    return True
                rgb, done = frame
                for msg in chunk_messages(rgb, 0):
                    try:
                        await self.send(msg)
                    except ConnectionError:
                        self.cancel.value = 1
                        return True
                if done >= total:
                    self.cancel.value = 1
                    return False
        finally:
            frames.close()


class AdaptiveJob:
    """A whole-frame job that renders to a per-pixel error target (rt_amd.render_to_error): two full
    passes, then sparse passes over the pixels whose estimated error is still above abs_tol, until none is left or every
    such pixel holds the request's spp. Every refined frame is sent again with the same chunk messages, as
    ProgressiveJob does. RenderJob's interface: a stop takes effect between passes, and inside a pass through the cancel
    word."""

    def __init__(self, send, abs_tol, first=16, device=0, batch=0, gain=None, **denoise_params):
        self.send = send
        self.abs_tol = abs_tol
        self.first = first
        self.device = device
        self.batch, self.gain = batch, gain  # RT_TARGET_BATCH: passed on to render_to_error only when set
        self.denoise_params = denoise_params
        self.cancel = ctypes.c_int32(1)  # starts cancelled == not running

    def running(self):
        return self.cancel.value == 0

    def stop(self):
        self.cancel.value = 1

    async def run(self, scene, width, height, spp, seed):
        """spp is the per-pixel budget. Returns True when stopped before the last frame was sent."""
        import rt_amd

        self.cancel.value = 0
        loop = asyncio.get_running_loop()
        batched = {}
        if self.batch:
            batched["batch"] = self.batch
            if self.gain is not None:
                batched["gain"] = self.gain
        frames = rt_amd.render_to_error(scene, width, height, abs_tol=self.abs_tol, max_spp=max(spp, self.first),
                                        first=self.first, seed=seed, device=self.device, cancel=self.cancel,
                                        **batched, **self.denoise_params)
        try:
            while True:
                if self.cancel.value:
                    return True
                frame = await loop.run_in_executor(None, next, frames, None)
                if frame is None or self.cancel.value:
                    return True
                rgb, _, active = frame
                for msg in chunk_messages(rgb, 0):
                    try:
                        await self.send(msg)
                    except ConnectionError:
                        self.cancel.value = 1
                        return True
                if active == 0.0:  # nothing left above the target or below the budget: the last frame
                    self.cancel.value = 1
                    return False
        finally:
            frames.close()


class InteractiveJob:
    """A whole-frame job whose connection keeps the last accumulator and view (rt_amd.render_interactive, DESIGN.md
    §14): a request for the scene the connection rendered last starts from the history reprojected into the new
    camera, at most max_n samples per subpixel of it; then two full-frame passes of `first` spp and, with abs_tol,
    sparse passes up to the request's spp per pixel. One frame is sent per request. A request for another scene or
    frame size starts over. RenderJob's interface; a stop ends the request and drops the history."""

    def __init__(self, send, max_n, first=8, abs_tol=None, device=0, **denoise_params):
        self.send = send
        self.max_n = max_n
        self.first = first
        self.abs_tol = abs_tol
        # RT_REPROJECT_FILL=<spp>[,<refresh>]: after the first request, two sparse passes of <spp> over the pixels
        # without history (and one over a refresh pattern) instead of the two full-frame passes
        self.fill_spp, self.refresh = parse_fill(os.environ.get("RT_REPROJECT_FILL"))
        self.device = device
        self.denoise_params = denoise_params
        self.cancel = ctypes.c_int32(1)  # starts cancelled == not running
        self._frames = None  # the running render_interactive generator and what it was made for
        self._key = None
        self._base = None
        self._next_view = None

    def running(self):
        return self.cancel.value == 0

    def stop(self):
        self.cancel.value = 1

    def _views(self):
        while True:  # read by render_interactive when a frame is asked for
            yield self._next_view

    def _drop(self):
        if self._frames is not None:
            self._frames.close()
        self._frames, self._key, self._base = None, None, None

    async def run(self, scene, width, height, spp, seed):
        """Returns True when stopped before the frame was sent."""
        import rt_amd

        self.cancel.value = 0
        loop = asyncio.get_running_loop()
        base = scene._base if scene._base is not None else scene
        key = (id(base), width, height)
        if self._frames is None or self._key != key:
            self._drop()
            self._frames = rt_amd.render_interactive(base, self._views(), width, height, first=self.first,
                                                     max_n=self.max_n, abs_tol=self.abs_tol, seed=seed,
                                                     device=self.device, cancel=self.cancel, fill_spp=self.fill_spp,
                                                     refresh=self.refresh, **self.denoise_params)
            self._key = key
            self._base = base  # keeps id(base) unique while the generator lives
        self._next_view = dict(scene.camera(), view_spp=spp)
        frame = await loop.run_in_executor(None, next, self._frames, None)
        if frame is None or self.cancel.value:
            self._drop()  # a cancelled generator has ended: the next request starts over
            self.cancel.value = 1
            return True
        for msg in chunk_messages(frame[0], 0):
            try:
                await self.send(msg)
            except ConnectionError:
                self.cancel.value = 1
                return True
        self.cancel.value = 1
        return False


class Server:
    def __init__(self, scenes, renderer=None, width=WIDTH, height=HEIGHT, band_rows=32, log=print, job_factory=None):
        self.scenes = scenes
        self.renderer = renderer or (gpu_band_renderer() if job_factory is None else None)
        self.width = width
        self.height = height
        self.band_rows = band_rows
        self.connections = set()
        self.log = log
        # job_factory(send) makes a connection's job (RenderJob's interface); None: RenderJob over `renderer`
        self.job_factory = job_factory

    def new_id(self):  # server.rs:63-78
        while True:
            cid = "".join(random.sample(string.ascii_lowercase, 5))
            if cid not in self.connections:
                self.connections.add(cid)
                return cid

    async def handle(self, request):
        from aiohttp import WSMsgType, web

        ws = web.WebSocketResponse()
        await ws.prepare(request)
        cid = self.new_id()
        self.log(f"[{cid}] Accepted connection.")
        job = self.job_factory(ws.send_bytes) if self.job_factory else RenderJob(ws.send_bytes, self.renderer,
                                                                                 self.band_rows)
        task = None
        try:
            async for msg in ws:
                if msg.type != WSMsgType.TEXT:
                    continue
                self.log(f"[{cid}] New message: '{msg.data}'")
                try:
                    m = json.loads(msg.data)
                    kind = m["type"]
                except (ValueError, KeyError, TypeError):
                    self.log(f"[{cid}] failed to parse message")
                    break  # the reference panics here (server.rs:92): the connection ends
                if kind == "render" and not job.running():
                    name, spp = m.get("scene"), m.get("spp")
                    if name not in self.scenes or not isinstance(spp, int):
                        self.log(f"[{cid}] bad render request {m!r}")
                        continue
                    scene = self.scenes[name]
                    try:
                        cam = parse_camera(m)
                        if cam is not None:
                            scene = scene.view(**cam)  # shares the scene's data; RtError for a degenerate camera
                    except Exception as e:  # noqa: BLE001 (a bad camera is logged, like a bad scene name)
                        self.log(f"[{cid}] bad render request {m!r}: {e}")
                        continue
                    seed = int.from_bytes(os.urandom(8), "little") if "RT_SEED" not in os.environ \
                        else int(os.environ["RT_SEED"], 0)
                    self.log(f"[{cid}] Rendering...")
                    task = asyncio.ensure_future(self._run(cid, job, scene, spp, seed))
                elif kind == "stop_rendering" and job.running():
                    job.stop()
                    self.log(f"[{cid}] Render cancelled.")
        finally:
            job.stop()
            if task is not None:
                await asyncio.gather(task, return_exceptions=True)
            self.connections.discard(cid)
            self.log(f"[{cid}] Disconnected.")
        return ws

    async def _run(self, cid, job, scene, spp, seed):
        cancelled = await job.run(scene, self.width, self.height, spp, seed)
        if not cancelled:
            self.log(f"[{cid}] Done rendering.")

    def app(self):
        from aiohttp import web

        app = web.Application()
        app.router.add_get("/", self.handle)
        return app


def main(argv=None):
    from aiohttp import web

    argv = argv if argv is not None else sys.argv[1:]
    if not argv:
        print("Usage: python -m rt_amd.server <scenes directory>", file=sys.stderr)
        return 2
    import rt_amd

    scene_dir = argv[0]
    scenes = {n: rt_amd.Scene.from_toml(os.path.join(scene_dir, f"{n}.toml")) for n in SCENE_NAMES}
    port = int(os.environ.get("PORT", "8080"))  # main.rs:38
    print(f"Listening on port {port}.")
    fp32 = os.environ.get("RT_PRECISION", "f64") == "f32"  # f64 (the reference's arithmetic) by default
    if fp32:
        # the f32 mode traces meshes with the nearest-triangle semantics
        # (geometry.rs:886-903), not the reference's first-hit octree walk (geometry.rs:1237-1295)
        print("RT_PRECISION=f32: f32 perf mode; meshes (flying_unicorn) use nearest-triangle hits, not the "
              "reference's octree semantics; frames differ statistically from server.rs", file=sys.stderr)
    if "RT_REPROJECT" in os.environ and ("RT_TARGET_ERROR" in os.environ or "RT_PROGRESSIVE" in os.environ):
        # orbiting: a connection keeps its accumulator and view; a new camera starts from the reprojected history
        max_n = int(os.environ["RT_REPROJECT"])
        abs_tol = float(os.environ["RT_TARGET_ERROR"]) if "RT_TARGET_ERROR" in os.environ else None
        first = int(os.environ.get("RT_PROGRESSIVE", rt_amd.ERROR_TARGET_DEFAULTS["first"]))
        print(f"RT_REPROJECT={max_n}: whole-frame jobs that inherit up to {max_n} samples per subpixel from the "
              f"connection's last view; two passes of {first} spp per request"
              + (f", then sparse passes to the error target {abs_tol} within the request's spp" if abs_tol is not None
                 else "")
              + (f"; RT_REPROJECT_FILL={os.environ['RT_REPROJECT_FILL']}: after a connection's first request the "
                 "two passes cover only the pixels without history" if "RT_REPROJECT_FILL" in os.environ else ""),
              file=sys.stderr)
        server = Server(scenes, job_factory=lambda send: InteractiveJob(send, max_n, first=first, abs_tol=abs_tol))
    elif "RT_TARGET_ERROR" in os.environ:
        # rendering to an error target: whole frames, sparse passes over the pixels still above it
        abs_tol = float(os.environ["RT_TARGET_ERROR"])
        first = int(os.environ.get("RT_PROGRESSIVE", rt_amd.ERROR_TARGET_DEFAULTS["first"]))
        batch, gain = parse_batch(os.environ.get("RT_TARGET_BATCH"))
        print(f"RT_TARGET_ERROR={abs_tol}: whole-frame jobs rendered to a per-pixel error target, first frame at "
              f"{first} spp, the request's spp as the per-pixel budget"
              + (f"; RT_TARGET_BATCH: up to {batch} passes per pixel in one launch" if batch else ""), file=sys.stderr)
        server = Server(scenes, job_factory=lambda send: AdaptiveJob(send, abs_tol, first=first, batch=batch, gain=gain))
    elif "RT_PROGRESSIVE" in os.environ:
        # progressive refinement: whole frames, each refined frame re-sent with the same chunk messages
        first = int(os.environ["RT_PROGRESSIVE"])
        print(f"RT_PROGRESSIVE={first}: whole-frame progressive jobs, first frame at {first} spp, variance-guided "
              "a-trous filter", file=sys.stderr)
        server = Server(scenes, job_factory=lambda send: ProgressiveJob(send, first=first))
    elif "RT_DENOISE" in os.environ:
        # denoised previews: whole frames (the filter needs an apron of 2 * (2^levels - 1) rows around a band)
        levels = int(os.environ["RT_DENOISE"])
        print(f"RT_DENOISE={levels}: whole-frame renders, {levels}-level a-trous filter", file=sys.stderr)
        server = Server(scenes, renderer=gpu_denoised_frame_renderer(levels=levels), band_rows=HEIGHT)
    else:
        server = Server(scenes, renderer=gpu_band_renderer(fp32=fp32))
    web.run_app(server.app(), host="0.0.0.0", port=port, print=None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
