"""Host-side mirror of fortio/tray's `ray` package API over the MI355X C-ABI.

Same names, field meanings and defaulting as the Go package, so code written
against `ray.New(w, h)` / `(*Tracer).Render(scene)` reads the same here:

    Go (ray/)                                   here (tray_amd.ray)
    New(w, h) *Tracer           tracer.go:38    New(w, h) -> Tracer
    (*Tracer).Render(*Scene)    tracer.go:48    Tracer.Render(scene) -> (H, W, 4) uint8 RGBA
    (*Tracer).RenderLines(...)  tracer.go:120   Tracer.RenderLines(idx, yStart, yEnd, scene)
    Camera / Initialize         camera.go:9,43  Camera / Camera.Initialize(w, h)
    RichSceneCamera()           camera.go:144   RichSceneCamera()
    Scene / Sphere / AmbientLight objects.go    Scene / Sphere / AmbientLight
    Lambertian/Metal/Dielectric materials.go    Lambertian / Metal / Dielectric
    DefaultScene(), RichScene(rng) objects.go   DefaultScene(), RichScene(seed)
    DefaultBackground()         objects.go:106  DefaultBackground()
    (*Camera).GetRay(...)       camera.go:113   Tracer.CameraRays(yStart, yEnd) -> (rays, ids), every sample's ray
    (*Scene).Hit(r, iv, hr)     objects.go:37   Scene.Hit(origins, directions, interval) -> HIT_DTYPE array
    (*Scene).RayColor(r, depth) objects.go:49   Scene.RayColor(origins, directions, depth, seed) -> (rgb, segments)
    Material.Scatter(r, rec)    materials.go:13 Scene.Scatter(origins, directions, hits, seed) -> SCATTER_DTYPE array
    AmbientLight.Hit(r)         objects.go:68   AmbientLight.Hit(directions) -> (n, 3) colours
    (no Go counterpart)                         Scene.Occluded(origins, directions, t_end) -> (n,) bool
    (no Go counterpart)                         Tracer.RenderAOV(scene) -> albedo, normal, depth, coverage, index
    (no Go counterpart)                         Tracer.Denoise(frame, aov) -> (H, W, 3) float64, the guided filter
    (no Go counterpart)                         Tracer.RenderDenoised(scene) -> (H, W, 4) uint8 RGBA, filtered on the device

The six from CameraRays to RenderAOV are batched (include/tray_query.h, tray_shade.h): arrays of rays in, arrays of
results out, each one kernel launch on the scene's device copy, which the Scene
keeps while its spheres and background do not change (a picking loop uploads
once). They take numpy arrays and stage them through torch tensors.

The hot loop (everything under RenderLines) runs in the gfx950 megakernel via
tray_amd._lib; this module only applies the Go defaults and marshals data.
Differences by design: RichScene takes a seed (the scene stream is the counter
RNG of include/tray.h, not fortio.org/rand), NumWorkers is kept for API parity
but the parallelism is the GPU grid, and `idx` of RenderLines is accepted and
ignored (draws are keyed by pixel, not by row chunk).
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib

Vec3 = tuple  # (x, y, z) — value semantics like the Go struct
ColorF = tuple


def _v(v) -> tuple:
    t = tuple(float(c) for c in v)
    if len(t) != 3:
        raise ValueError("expected 3 components")
    return t


# ------------------------------------------------------------------ materials
@dataclass(frozen=True)
class Lambertian:  # ray/materials.go:9-11
    Albedo: ColorF = (0.0, 0.0, 0.0)


@dataclass(frozen=True)
class Metal:  # ray/materials.go:23-26
    Albedo: ColorF = (0.0, 0.0, 0.0)
    Fuzz: float = 0.0


@dataclass(frozen=True)
class Dielectric:  # ray/materials.go:40-42
    RefIdx: float = 1.0


@dataclass
class Sphere:  # ray/objects.go:75-79
    Center: Vec3
    Radius: float
    Mat: object


@dataclass
class AmbientLight:  # ray/objects.go:64-66
    ColorA: ColorF = (0.0, 0.0, 0.0)
    ColorB: ColorF = (0.0, 0.0, 0.0)

    def Hit(self, directions, device: int = 0) -> np.ndarray:  # ray/objects.go:68-73
        """AmbientLight.Hit for n rays of the given (n, 3) directions: (n, 3) float64
        colours (a zero direction gives NaN, as in Go). Needs no scene."""
        d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
        torch, rays = _stage_rays(np.zeros_like(d), d, device)
        n = rays.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float64, device=rays.device)
        _lib.background_hit_async(_background(self), rays.data_ptr(), n, rgb.data_ptr(), device,
                                  torch.cuda.current_stream(rays.device).cuda_stream)
        return rgb.cpu().numpy()


def DefaultBackground() -> AmbientLight:  # ray/objects.go:106-110
    return AmbientLight((1.0, 1.0, 1.0), (0.4, 0.65, 1.0))


@dataclass
class Scene:  # ray/objects.go:32-35
    Objects: list = field(default_factory=list)
    Background: AmbientLight = field(default_factory=AmbientLight)
    _uploaded: dict = field(default_factory=dict, repr=False, compare=False)  # device -> (scene bytes, DeviceScene)

    def _device_scene(self, device: int) -> "_lib.DeviceScene":
        """The scene's copy on `device` for the batched queries: uploaded on first
        use and again only when the spheres or the background have changed."""
        arr = self.to_array()
        bg = _background(self.Background)
        key = arr.tobytes() + bytes(bg)
        have = self._uploaded.get(device)
        if have is not None and have[0] == key:
            return have[1]
        if have is not None:
            have[1].release()
        dev = _lib.DeviceScene(arr, bg, device)
        self._uploaded[device] = (key, dev)
        return dev

    def _geometry(self) -> np.ndarray:
        """(n, 4) float64: centre and radius per object, as to_array() flattens them."""
        arr = self.to_array()
        return np.ascontiguousarray(np.concatenate([arr["center"].reshape(-1, 3), arr["radius"].reshape(-1, 1)],
                                                   axis=1))

    def _set_geometry(self, geometry: np.ndarray) -> None:
        for o, g in zip(self.Objects, geometry):
            o.Center = (float(g[0]), float(g[1]), float(g[2]))
            o.Radius = float(g[3])

    def _adopt(self, device: int, dev: "_lib.DeviceScene | None") -> None:
        """`dev` now holds the scene as Objects and Background describe it (None: nothing does)."""
        if dev is None:
            self._uploaded.pop(device, None)
        else:
            self._uploaded[device] = (self.to_array().tobytes() + bytes(_background(self.Background)), dev)

    def Move(self, centers, radii=None, device: int = 0) -> bool:
        """New centres ((n, 3)) and, unless None, radii ((n,)) for the scene's spheres, in list
        order: sets Center and Radius on Objects and, when the scene has an up-to-date copy on
        `device`, moves that copy's spheres in place and refits its BVH there
        (include/tray_scene_update.h) instead of uploading again, so the next query or render
        reuses it. Returns whether that happened: False when there was no such copy, or when the
        update was refused (a sphere left the uploaded scene's bound, or is NaN or infinite on a
        scene with a tree); the copy is then released and the next use uploads afresh. Either way
        the results are those of a new Scene with the same spheres. No Go counterpart."""
        c = np.asarray(centers, dtype=np.float64)
        n = len(self.Objects)
        if c.shape != (n, 3):
            raise ValueError(f"centers must be ({n}, 3); got {c.shape}")
        have = self._uploaded.get(device)
        if have is not None and have[0] != self.to_array().tobytes() + bytes(_background(self.Background)):
            have[1].release()  # stale already: something else changed since the upload
            self._adopt(device, None)
            have = None
        geometry = self._geometry()
        geometry[:, :3] = c
        if radii is not None:
            r = np.asarray(radii, dtype=np.float64)
            if r.shape != (n,):
                raise ValueError(f"radii must be ({n},); got {r.shape}")
            geometry[:, 3] = r
        self._set_geometry(geometry)
        if have is None:
            return False
        if n == 0:  # nothing to move
            return True
        if have[1].update(geometry).applied:
            self._adopt(device, have[1])
            return True
        have[1].release()
        self._adopt(device, None)
        return False

    def Hit(self, origins, directions, interval=(1e-6, math.inf), device: int = 0) -> np.ndarray:  # ray/objects.go:37-46
        """Scene.Hit for n rays ((n, 3) origins and directions) over Interval{1e-6,
        interval[1]}: a _lib.HIT_DTYPE array (index -1: no hit). The interval
        start is the renderer's FrontEpsilon.Start; any other raises."""
        if float(interval[0]) != 1e-6:
            raise _lib.TrayError(_lib.TRAY_ERR_INVALID_ARGUMENT,
                                 "Scene.Hit: the interval start is fixed at 1e-6 (FrontEpsilon.Start, ray/vec3.go:218)")
        torch, rays = _stage_rays(origins, directions, device)
        n = rays.shape[0]
        hits = torch.empty((n, _lib.HIT_DTYPE.itemsize // 8), dtype=torch.float64, device=rays.device)
        dev = self._device_scene(device)
        dev.hit_async(rays.data_ptr(), n, hits.data_ptr(), float(interval[1]),
                      stream=torch.cuda.current_stream(rays.device).cuda_stream)
        return hits.cpu().numpy().reshape(-1).view(_lib.HIT_DTYPE)

    def RayColor(self, origins, directions, depth: int, seed: int, ids=None, device: int = 0):  # ray/objects.go:49-62
        """Scene.RayColor(r, depth) for n rays: ((n, 3) float64 colours, (n,) uint32
        Scene.Hit counts). ids ((n, 2) uint32, e.g. from Tracer.CameraRays): the
        (pixel, sample word) whose scatter draws each ray takes under `seed`;
        None: pixel = ray index, sample 0."""
        torch, rays = _stage_rays(origins, directions, device)
        n = rays.shape[0]
        ids_t = None
        if ids is not None:
            ids_np = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if ids_np.size != 2 * n:
                raise ValueError("ids must hold a (pixel, sample) pair per ray")
            ids_t = torch.from_numpy(ids_np.view(np.int32)).to(rays.device)
        rgb = torch.empty((n, 3), dtype=torch.float64, device=rays.device)
        seg = torch.empty((n,), dtype=torch.int32, device=rays.device)
        dev = self._device_scene(device)
        dev.ray_color_async(rays.data_ptr(), n, int(depth), int(seed), rgb.data_ptr(),
                            ids_t.data_ptr() if ids_t is not None else None, seg.data_ptr(),
                            stream=torch.cuda.current_stream(rays.device).cuda_stream)
        return rgb.cpu().numpy(), seg.cpu().numpy().view(np.uint32)

    def Scatter(self, origins, directions, hits, seed: int, ids=None, bounce: int = 0,
                device: int = 0) -> np.ndarray:  # ray/materials.go:13-64
        """hits[i].Mat.Scatter(ray i, hits[i]) for n rays: a _lib.SCATTER_DTYPE array
        (scattered 0: absorbed or no hit, every other field zero). hits: a
        _lib.HIT_DTYPE array of the same length, e.g. Scene.Hit's; point, normal,
        front_face and index are read from it. ids and seed as for RayColor; the
        draws are those of `bounce`."""
        o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        h = np.ascontiguousarray(hits)
        if h.dtype != _lib.HIT_DTYPE:
            raise TypeError("hits must use tray_amd._lib.HIT_DTYPE")
        h = h.reshape(-1)
        if len(h) != len(o):
            raise ValueError("hits must hold one record per ray")
        ids_np = None
        if ids is not None:
            ids_np = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if ids_np.size != 2 * len(o):
                raise ValueError("ids must hold a (pixel, sample) pair per ray")
        torch, rays = _stage_rays(o, directions, device)
        n = rays.shape[0]
        hits_t = torch.from_numpy(h.view(np.float64).reshape(n, _lib.HIT_DTYPE.itemsize // 8)).to(rays.device)
        ids_t = torch.from_numpy(ids_np.view(np.int32)).to(rays.device) if ids_np is not None else None
        out = torch.empty((n, _lib.SCATTER_DTYPE.itemsize // 8), dtype=torch.float64, device=rays.device)
        dev = self._device_scene(device)
        dev.scatter_async(rays.data_ptr(), hits_t.data_ptr(), n, int(seed), out.data_ptr(),
                          ids_t.data_ptr() if ids_t is not None else None, int(bounce),
                          stream=torch.cuda.current_stream(rays.device).cuda_stream)
        return out.cpu().numpy().reshape(-1).view(_lib.SCATTER_DTYPE)

    def Occluded(self, origins, directions, t_end=math.inf, device: int = 0) -> np.ndarray:
        """Whether anything lies in (1e-6, t_end) along each of n rays: (n,) bool,
        Scene.Hit(...)["index"] >= 0 at one byte per ray and with a traversal that
        stops at the first root. t_end: a scalar, or an (n,) array of per-ray ends
        (NaN or <= 1e-6: an empty interval, False)."""
        o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        ends = None
        if np.ndim(t_end) > 0:
            ends = np.ascontiguousarray(t_end, dtype=np.float64).reshape(-1)
            if len(ends) != len(o):
                raise ValueError("t_end must be a scalar or hold one end per ray")
        torch, rays = _stage_rays(o, directions, device)
        n = rays.shape[0]
        ends_t = torch.from_numpy(ends).to(rays.device) if ends is not None else None
        out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        dev = self._device_scene(device)
        dev.occluded_async(rays.data_ptr(), n, out.data_ptr(), math.inf if ends is not None else float(t_end),
                           ends_t.data_ptr() if ends_t is not None else None,
                           stream=torch.cuda.current_stream(rays.device).cuda_stream)
        return out.cpu().numpy().astype(bool)

    def to_array(self) -> np.ndarray:
        """Flatten to the C-ABI's tray_sphere array; unsupported objects raise
        (the Go Hittable/Material interfaces are open, the device path is not)."""
        out = np.zeros(len(self.Objects), dtype=_lib.SPHERE_DTYPE)
        for i, o in enumerate(self.Objects):
            if not isinstance(o, Sphere):
                raise _lib.TrayError(_lib.TRAY_ERR_UNSUPPORTED, f"object {i} is not a Sphere")
            out[i]["center"] = _v(o.Center)
            out[i]["radius"] = float(o.Radius)
            m = o.Mat
            if isinstance(m, Lambertian):
                out[i]["material"], out[i]["albedo"] = _lib.LAMBERTIAN, _v(m.Albedo)
            elif isinstance(m, Metal):
                out[i]["material"], out[i]["albedo"], out[i]["param"] = _lib.METAL, _v(m.Albedo), float(m.Fuzz)
            elif isinstance(m, Dielectric):
                out[i]["material"], out[i]["param"] = _lib.DIELECTRIC, float(m.RefIdx)
            else:
                raise _lib.TrayError(_lib.TRAY_ERR_UNSUPPORTED, f"object {i}: unsupported material {type(m)}")
        return out

    @staticmethod
    def from_array(spheres: np.ndarray, background: AmbientLight | None = None) -> "Scene":
        objs = []
        for s in spheres:
            kind = int(s["material"])
            if kind == _lib.LAMBERTIAN:
                mat = Lambertian(tuple(s["albedo"].tolist()))
            elif kind == _lib.METAL:
                mat = Metal(tuple(s["albedo"].tolist()), float(s["param"]))
            else:
                mat = Dielectric(float(s["param"]))
            objs.append(Sphere(tuple(s["center"].tolist()), float(s["radius"]), mat))
        return Scene(objs, background or AmbientLight())


def _stage_rays(origins, directions, device: int):
    """(torch, an (n, 6) float64 tensor on `device` laid out as n x tray_ray)."""
    import torch

    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions must both be (n, 3)")
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    return torch, torch.from_numpy(rays).to(f"cuda:{int(device)}")


def _background(bg: AmbientLight) -> _lib.Background:
    return _lib.Background((ctypes.c_double * 3)(*_v(bg.ColorA)), (ctypes.c_double * 3)(*_v(bg.ColorB)))


def DefaultScene() -> Scene:  # ray/objects.go:112-130
    arr = np.zeros(5, dtype=_lib.SPHERE_DTYPE)
    n = ctypes.c_int32()
    _lib.check(_lib.lib().tray_default_scene(arr.ctypes.data, 5, ctypes.byref(n)))
    return Scene.from_array(arr[: n.value], DefaultBackground())


def rich_scene_array(seed: int, half_extent: int = 11) -> np.ndarray:
    cap = _lib.lib().tray_rich_scene_capacity(half_extent)
    arr = np.zeros(cap, dtype=_lib.SPHERE_DTYPE)
    n = ctypes.c_int32()
    _lib.check(_lib.lib().tray_rich_scene(int(seed) & (2**64 - 1), half_extent, arr.ctypes.data, cap,
                                          ctypes.byref(n)))
    return arr[: n.value].copy()


def RichScene(seed: int, half_extent: int = 11) -> Scene:  # ray/objects.go:132-175
    """Book-cover scene; Background left zero like the Go function (Render defaults it)."""
    return Scene.from_array(rich_scene_array(seed, half_extent))


# --------------------------------------------------------------------- camera
@dataclass
class Camera:  # ray/camera.go:9-39
    Position: Vec3 = (0.0, 0.0, 0.0)
    LookAt: Vec3 = (0.0, 0.0, 0.0)
    Up: Vec3 = (0.0, 0.0, 0.0)
    VerticalFoV: float = 0.0
    FocalLength: float = 0.0
    FocusDistance: float = 0.0
    Aperture: float = 0.0
    _state: _lib.CameraState | None = field(default=None, repr=False, compare=False)

    def Initialize(self, width: int, height: int) -> None:  # ray/camera.go:43-105
        cs = _lib.CameraSetup((ctypes.c_double * 3)(*_v(self.Position)), (ctypes.c_double * 3)(*_v(self.LookAt)),
                              (ctypes.c_double * 3)(*_v(self.Up)), float(self.VerticalFoV),
                              float(self.FocalLength), float(self.FocusDistance), float(self.Aperture))
        st = _lib.CameraState()
        _lib.check(_lib.lib().tray_camera_initialize(ctypes.byref(cs), width, height, ctypes.byref(st)))
        self.Position, self.LookAt, self.Up = tuple(cs.position), tuple(cs.look_at), tuple(cs.up)
        self.VerticalFoV, self.FocalLength = cs.vertical_fov, cs.focal_length
        self.FocusDistance, self.Aperture = cs.focus_distance, cs.aperture
        self._state = st

    # computed fields, named as in camera.go:34-39
    @property
    def pixel00(self) -> Vec3:
        return tuple(self._state.pixel00)

    @property
    def pixelXVector(self) -> Vec3:
        return tuple(self._state.pixel_x)

    @property
    def pixelYVector(self) -> Vec3:
        return tuple(self._state.pixel_y)

    @property
    def defocusDiskU(self) -> Vec3:
        return tuple(self._state.defocus_u)

    @property
    def defocusDiskV(self) -> Vec3:
        return tuple(self._state.defocus_v)


def RichSceneCamera() -> Camera:  # ray/camera.go:144-154
    cs = _lib.CameraSetup()
    _lib.check(_lib.lib().tray_rich_scene_camera(ctypes.byref(cs)))
    return Camera(tuple(cs.position), tuple(cs.look_at), tuple(cs.up), cs.vertical_fov, cs.focal_length,
                  cs.focus_distance, cs.aperture)


def orbit_position(position: Vec3, look_at: Vec3, up: Vec3, degrees: float) -> Vec3:
    """`position` turned about `look_at` around the axis `up` by `degrees` (Rodrigues' rotation; an
    all-zero `up` means (0, 1, 0), as Camera.Initialize defaults it)."""
    k = np.asarray(up, dtype=np.float64)
    if not k.any():
        k = np.array([0.0, 1.0, 0.0])
    k = k / math.sqrt(float(k @ k))
    v = np.asarray(position, dtype=np.float64) - np.asarray(look_at, dtype=np.float64)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    r = v * c + np.cross(k, v) * s + k * (float(k @ v) * (1.0 - c))
    return tuple((r + np.asarray(look_at, dtype=np.float64)).tolist())


def Orbit(camera: Camera, degrees: float) -> Camera:
    """A copy of `camera` turned about its LookAt around its Up axis by `degrees` (not initialized)."""
    return Camera(orbit_position(camera.Position, camera.LookAt, camera.Up, degrees), tuple(camera.LookAt),
                  tuple(camera.Up), camera.VerticalFoV, camera.FocalLength, camera.FocusDistance, camera.Aperture)


ORBIT_STEP_DEGREES = 1.0  # the CLI's default -orbit-step (tools/temporal_sweep.py)
REFILL_DEFAULT = 3  # the CLI's -refill without a number (tools/temporal_variance_sweep.py)
BOUNCE_STEP = 0.4  # the CLI's -bounce: radians of every sphere's phase between frames


def Bounce(scene: Scene, frames: int, step: float = BOUNCE_STEP) -> np.ndarray:
    """The geometries of `frames` frames for Tracer.RenderAnimation, (frames, n, 4) float64: the
    spheres of `scene` with a radius below 0.5 hop above the ground, y = R + |sin(i + step x frame)|
    for the sphere at list index i; everything else stays where it is."""
    g = scene._geometry()
    out = np.repeat(g[None], int(frames), axis=0)
    small = np.nonzero(g[:, 3] < 0.5)[0]
    for k in range(int(frames)):
        out[k, small, 1] = g[small, 3] + np.abs(np.sin(small + step * k))
    return out

# --------------------------------------------------------------------- tracer
_CAMERA_FIELDS = ("Position", "LookAt", "Up", "VerticalFoV", "FocalLength", "FocusDistance", "Aperture")
_GUIDES = (("albedo", 3), ("normal", 3), ("depth", 1))  # the filters' guides: name, channels


def _guide_ptrs(aov: dict) -> list:
    """The device pointers of the guides in `aov`, in the C calls' order; None where it has none."""
    return [aov[name].data_ptr() if aov.get(name) is not None else None for name, _ in _GUIDES]


def _given(**kw) -> dict:
    """The arguments that are not None: the library's defaults stand for the others."""
    return {name: value for name, value in kw.items() if value is not None}


def _refill_options(refill, refill_tolerance, refill_dilate) -> tuple:
    """(refill as an int, refill_tolerance as a float) of RenderSequence's and RenderAnimation's
    arguments; ValueError for what they refuse."""
    if isinstance(refill, bool) or not isinstance(refill, (int, np.integer)) or refill < 0:
        raise ValueError("refill must be an integer >= 0")
    if refill_dilate not in (0, 1):
        raise ValueError("refill_dilate must be 0 or 1")
    rt = float(refill_tolerance)
    if not (rt >= 0.0 and rt * rt < float("inf")):
        raise ValueError("refill_tolerance must be finite and >= 0, with a finite square")
    return int(refill), rt


def _temporal_options(overrides: dict, refill: int) -> "_lib.TemporalParams":
    """tray_temporal_params with the same methods' overrides; ValueError for an unknown one and for a
    refill that max_history leaves no room for."""
    unknown = sorted(set(overrides) - {n for n, _ in _lib.TemporalParams._fields_})
    if unknown or "reserved" in overrides:
        raise ValueError(f"unknown temporal parameters {unknown or ['reserved']}")
    tp = _lib.temporal_params(**overrides)
    if refill and tp.max_history < 1 + refill:
        raise ValueError(f"refill={refill} needs max_history >= {1 + refill}: no pixel could hold "
                         f"1 + refill frames (max_history is {tp.max_history})")
    return tp


class _TemporalLoop:
    """The frame body Tracer.RenderSequence and Tracer.RenderAnimation(temporal=True) share: the
    buffers of `count` frames (two ping-pong states, the frame, the records, the RGBA frames, with
    `variance` the variance plane, with `refill` the selection's workspace and the list renderer's
    values, with `denoise` the guides), one frame enqueued on `stream` per call of frame(), and the
    readback into the tracer's fields in finish()."""

    def __init__(self, tracer, torch, device, where, stream, count, tp, variance, refill, refill_tolerance,
                 refill_dilate, denoise):
        self.t, self.torch, self.device, self.where, self.stream = tracer, torch, device, where, stream
        self.count, self.tp, self.variance, self.refill, self.denoise = count, tp, variance, refill, denoise
        h, w = tracer.height, tracer.width
        f64 = dict(dtype=torch.float64, device=where)

        def planes():
            t = dict(colour=torch.empty((h, w, 3), **f64), age=torch.empty((h, w), dtype=torch.int32, device=where),
                     index=torch.empty((h, w), dtype=torch.int32, device=where), depth=torch.empty((h, w), **f64))
            if variance:
                t["m2"] = torch.empty((h, w, 3), **f64)
                return t, _lib.TemporalVarState(t["colour"].data_ptr(), t["m2"].data_ptr(), t["age"].data_ptr(),
                                                t["index"].data_ptr(), t["depth"].data_ptr(), w, h)
            return t, _lib.TemporalState(t["colour"].data_ptr(), t["age"].data_ptr(), t["index"].data_ptr(),
                                         t["depth"].data_ptr(), w, h)

        self.states = [planes(), planes()]
        self.frame_buffer = torch.empty((h, w, 3), **f64)
        self.records = torch.empty((count, 2), dtype=torch.int64, device=where)
        self.rgba = torch.empty((count, h, w, 4), dtype=torch.uint8, device=where)
        self.aov = tracer._guide_buffers(torch, where) if denoise else None
        self.var_plane = torch.empty((h, w, 3), **f64) if variance else None
        if refill:
            self.ap = _lib.adaptive_params(tolerance=refill_tolerance, min_passes=1 + refill,
                                           max_passes=int(tp.max_history), dilate=int(refill_dilate))
            self.nbytes = _lib.adaptive_workspace_bytes(w, h)
            self.work = torch.empty((self.nbytes // 8,), **f64)
            self.active = torch.empty((h * w,), dtype=torch.int32, device=where)
            self.arecord = torch.empty((4,), **f64)
            self.values = torch.empty((refill * h * w * 3,), **f64)  # frame 0 lists every pixel
        self.stride = 1 + refill  # frame k owns the passes k * stride .. (k + 1) * stride - 1
        self.refilled = []
        self.shown = None

    def _as_var_state(self, st):
        """A state for tray_temporal_motion_step_async: a plain one widened with a null m2."""
        if isinstance(st, _lib.TemporalVarState):
            return st
        return _lib.TemporalVarState(st.colour, None, st.age, st.index, st.depth, st.width, st.height)

    def frame(self, k, dev, cam, prev_cam, prev_geometry=None):
        """Frame k through `cam` on the scene copy `dev`: the render, the step from the state of frame
        k - 1 (seen through prev_cam; None for k = 0), the refill chain, the filter and the encoding.
        prev_geometry: None for a scene that has not changed since frame k - 1, else (the device
        pointer of what the scene held then, n): the step then follows the moved spheres
        (include/tray_temporal_motion.h)."""
        t, torch, device, stream, tp, refill = self.t, self.torch, self.device, self.stream, self.tp, self.refill
        h, w = t.height, t.width
        frame, states, records, var_plane = self.frame_buffer, self.states, self.records, self.var_plane
        params = t._params(t.seed, k * self.stride)
        dev.render_async(cam._state, params, frame.data_ptr(), None, stream)
        out = states[k & 1]
        history = states[(k - 1) & 1][1] if k else None
        if prev_geometry is not None:
            _lib.temporal_motion_step_async(dev.handle, cam._state, prev_cam._state if k else None,
                                            prev_geometry[0] if k else None, prev_geometry[1], tp, frame.data_ptr(),
                                            self._as_var_state(history) if k else None, self._as_var_state(out[1]),
                                            var_plane.data_ptr() if self.variance else None, None,
                                            records[k].data_ptr(), stream)
        elif self.variance:
            _lib.temporal_var_step_async(dev.handle, cam._state, prev_cam._state if k else None, tp,
                                         frame.data_ptr(), history, out[1],
                                         var_plane.data_ptr(), records[k].data_ptr(), stream)
        else:
            _lib.temporal_step_async(dev.handle, cam._state, prev_cam._state if k else None, tp,
                                     frame.data_ptr(), history, out[1],
                                     records[k].data_ptr(), stream)
        if refill:
            ast = out[1].adaptive()
            _lib.adaptive_select_async(ast, self.ap, self.active.data_ptr(), self.arecord.data_ptr(),
                                       self.work.data_ptr(), self.nbytes, None, device, stream)
            n_active = int(self.arecord.cpu().numpy().view(_lib.ADAPTIVE_RECORD_DTYPE)[0]["n_active"])  # 32 bytes
            self.refilled.append(n_active)
            if n_active:
                dev.render_pixels_async(cam._state, t._params(t.seed, k * self.stride + 1), self.active.data_ptr(),
                                        n_active, self.values.data_ptr(), refill, stream=stream)
                _lib.adaptive_fold_async(ast, self.active.data_ptr(), n_active, self.values.data_ptr(), refill, device,
                                         stream)
                _lib.temporal_var_variance_async(out[1], self.active.data_ptr(), n_active, var_plane.data_ptr(),
                                                 device, stream)
        shown = out[0]["colour"]
        if self.denoise:
            dev.render_aov_async(cam._state, params, *_guide_ptrs(self.aov), stream=stream)
            if self.variance:
                shown = t._denoise_variance_device(torch, shown, var_plane, self.aov, {})
            else:
                shown = t._denoise_device(torch, shown, self.aov, {})
        _lib.linear_to_srgba_async(shown.data_ptr(), h * w, self.rgba[k].data_ptr(), device, stream)
        self.shown = shown

    def finish(self) -> list:
        """Reads the last state, the records and the frames back into the tracer's fields; the frames."""
        t, count, refill = self.t, self.count, self.refill
        h, w = t.height, t.width
        last = self.states[(count - 1) & 1][0]
        if self.denoise:
            t.filtered = self.shown.cpu().numpy()  # the last frame as shown, before the sRGB encoding
        t.linear[:] = last["colour"].cpu().numpy()
        t.age = last["age"].cpu().numpy()
        if self.variance:
            t.variance = self.var_plane.cpu().numpy()
            t.m2 = last["m2"].cpu().numpy()
            t.refilled = self.refilled if refill else [0] * count
            t.pixel_passes = h * w * count + refill * sum(t.refilled)
        rec = self.records.cpu().numpy()
        t.fresh = [int(r[0]) for r in rec]
        t.mean_age = [float(r[1]) / (h * w) for r in rec]
        frames = [f.copy() for f in self.rgba.cpu().numpy()]
        t.imageData[:] = frames[-1]
        return frames


class Tracer:  # ray/tracer.go:25-36
    """Go's Tracer embeds Camera: t.Position etc. forward to t.Camera."""

    def __init__(self, width: int, height: int):
        object.__setattr__(self, "Camera", Camera())
        self.MaxDepth = 0
        self.NumRaysPerPixel = 0
        self.RayRadius = 0.0
        self.NumWorkers = 0
        self.ProgressFunc = None
        self.Seed = 0
        self.Device = 0  # which gfx950 device renders (no Go counterpart)
        self.Devices = None  # several devices: rows split over them (tray_render_devices; no Go counterpart)
        self.width = width
        self.height = height
        self.imageData = np.zeros((height, width, 4), dtype=np.uint8)  # image.NewRGBA, tracer.go:43
        self.linear = np.zeros((height, width, 3), dtype=np.float64)   # FP64 mean colour (parity format)
        self.segments = np.zeros((height, width), dtype=np.uint32)     # Scene.Hit calls per pixel

    def __getattr__(self, name):
        if name in _CAMERA_FIELDS:
            return getattr(object.__getattribute__(self, "Camera"), name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _CAMERA_FIELDS:
            setattr(self.Camera, name, value)
        else:
            object.__setattr__(self, name, value)

    def _apply_defaults(self, scene: Scene | None) -> Scene:  # ray/tracer.go:50-79
        if scene is None:
            scene = DefaultScene()
            self.Position = (-2.0, 2.0, 1.0)
            self.LookAt = (0.0, 0.0, -1.0)
            self.VerticalFoV = 20.0
            self.Aperture = 0.1
            d = [p - q for p, q in zip(self.Position, self.LookAt)]
            self.FocusDistance = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        zero = (0.0, 0.0, 0.0)
        if tuple(scene.Background.ColorA) == zero and tuple(scene.Background.ColorB) == zero:
            scene.Background = DefaultBackground()
        if self.MaxDepth <= 0:
            self.MaxDepth = 10
        if self.NumRaysPerPixel <= 0:
            self.NumRaysPerPixel = 1
        if self.RayRadius <= 0:
            self.RayRadius = 0.5
        if self.NumWorkers <= 0:
            self.NumWorkers = os.cpu_count() or 1  # runtime.GOMAXPROCS(0)
        return scene

    def _seed(self) -> int:
        # Seed 0 means "randomized each time" (tracer.go:33).
        return self.Seed if self.Seed else int.from_bytes(os.urandom(8), "little") or 1

    # ---- what the device-side methods below share: a new one is built from these ----
    def _target(self):
        """Where those methods run: torch, the device's index, its torch.device and the current
        stream there (which initializes the device: call it once the arguments are checked)."""
        import torch

        device = int(self.Devices[0] if self.Devices else self.Device)
        where = torch.device(f"cuda:{device}")
        return torch, device, where, torch.cuda.current_stream(where).cuda_stream

    def _params(self, seed: int, pass_: int = 0, flags: int = 0, y0: int = 0, y1: int | None = None):
        """The tracer's tray_params for progressive pass `pass_` of rows [y0, y1), the frame's by default."""
        return _lib.make_params(self.width, self.height, self.MaxDepth, self.NumRaysPerPixel, self.RayRadius, seed,
                                y0, y1, flags=flags, pass_=pass_)

    def _guide_buffers(self, torch, where) -> dict:
        """Device buffers for the filters' three guides over the frame, for tray_render_aov_async."""
        return {name: torch.empty((self.height, self.width, 3)[: 3 if ch > 1 else 2], dtype=torch.float64,
                                  device=where) for name, ch in _GUIDES}

    def _upload_guides(self, guides: dict, rows: int) -> dict:
        """A caller's host guides (as RenderAOV returns; a missing or None entry drops its term)
        as device tensors. Each must cover `rows` rows of the image's width: else ValueError,
        before any device work."""
        host = {}
        for name, ch in _GUIDES:
            g = guides.get(name)
            if g is None:
                continue
            g = np.ascontiguousarray(g, dtype=np.float64)
            if g.shape != (rows, self.width) + ((3,) if ch == 3 else ()):
                raise ValueError(f"{name} must cover the frame's {rows} rows of {self.width} pixels; got {g.shape}")
            host[name] = g
        if rows * self.width == 0:
            return {}
        torch, _, where, _ = self._target()
        return {name: torch.from_numpy(g).to(where) for name, g in host.items()}

    def _frame_guides(self, torch, dev, guides: dict | None, where, stream) -> dict:
        """The device guides for a filter over the whole frame: the caller's `guides` or, when
        None, the feature buffers of pass 0 of `seed` (tray_render_aov_async on `stream`)."""
        if guides is not None:
            return self._upload_guides(guides, self.height)
        aov = self._guide_buffers(torch, where)
        dev.render_aov_async(self.Camera._state, self._params(self.seed), *_guide_ptrs(aov), stream=stream)
        return aov

    def _show(self, torch, shown, device: int, stream) -> np.ndarray:
        """ColorF.ToSRGBA of the device frame `shown` (tray_linear_to_srgba_async) and the readback:
        `linear` holds `shown` and imageData, which is returned, its (H, W, 4) uint8 RGBA."""
        rgba = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=shown.device)
        _lib.linear_to_srgba_async(shown.data_ptr(), self.height * self.width, rgba.data_ptr(), device, stream)
        self.linear[:] = shown.cpu().numpy()
        self.imageData[:] = rgba.cpu().numpy()
        return self.imageData

    def _render_rows(self, y0: int, y1: int, scene: Scene) -> None:
        params = self._params(self._seed(), y0=y0, y1=y1)
        progress = None
        if self.ProgressFunc is not None:  # per row, while the device renders (tracer.go:126-128)
            def progress(rows):
                for _ in range(rows):
                    self.ProgressFunc(self.width)
        if self.Devices and len(self.Devices) > 1:  # one process, several GPUs, live progress from all of them
            rgb, seg = _lib.render_devices(scene.to_array(), _background(scene.Background), self.Camera._state,
                                           params, list(self.Devices), segments=True, progress=progress)
        else:
            rgb, seg = _lib.render(scene.to_array(), _background(scene.Background), self.Camera._state, params,
                                   self.Devices[0] if self.Devices else self.Device, segments=True,
                                   progress=progress)
        self.linear[y0:y1] = rgb
        self.segments[y0:y1] = seg
        rgba = np.zeros((y1 - y0, self.width, 4), dtype=np.uint8)
        _lib.check(_lib.lib().tray_to_srgba(rgb.ctypes.data, rgb.shape[0] * rgb.shape[1], rgba.ctypes.data))
        self.imageData[y0:y1] = rgba

    def CameraRays(self, yStart: int, yEnd: int, pass_: int = 0):  # ray/camera.go:113-142, ray/tracer.go:130-141
        """Camera.GetRay for every sample of rows [yStart, yEnd): the rays RenderLines
        traces there with the current (initialized) camera and fields, as a
        _lib.RAY_DTYPE array of (yEnd - yStart) x width x NumRaysPerPixel rays (row,
        column, sample order), and their (pixel, sample word) pairs as an (n, 2)
        uint32 array for Scene.RayColor. Set Seed for rays that repeat."""
        if self.Camera._state is None:
            raise _lib.TrayError(_lib.TRAY_ERR_INVALID_ARGUMENT, "Camera.Initialize must be called first")
        params = _lib.make_params(self.width, self.height, max(self.MaxDepth, 1), max(self.NumRaysPerPixel, 1),
                                  self.RayRadius if self.RayRadius > 0 else 0.5, self._seed(), yStart, yEnd,
                                  pass_=pass_)
        n = _lib.camera_rays_count(params)
        torch, device, where, stream = self._target()
        rays = torch.empty((n, 6), dtype=torch.float64, device=where)
        ids = torch.empty((n, 2), dtype=torch.int32, device=where)
        _lib.camera_rays_async(self.Camera._state, params, rays.data_ptr(), ids.data_ptr(), device, stream)
        return rays.cpu().numpy().reshape(-1).view(_lib.RAY_DTYPE), ids.cpu().numpy().view(np.uint32)

    def Render(self, scene: Scene | None) -> np.ndarray:  # ray/tracer.go:48-118
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        self._render_rows(0, self.height, scene)
        return self.imageData

    def RenderAOV(self, scene: Scene | None, yStart: int = 0, yEnd: int | None = None, pass_: int = 0) -> dict:
        """The first-hit feature buffers (include/tray_aov.h) of rows [yStart, yEnd) of the
        frame Render(scene) draws, with Render's defaulting: a dict of numpy arrays, albedo
        and normal (rows, W, 3) float64, depth and coverage (rows, W) float64, index
        (rows, W) int32 (-1: sample 0 misses). One fused launch over the frame's own camera
        rays of pass `pass_`; no Go counterpart. Set Seed for buffers that match a render."""
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        params = self._params(self._seed(), pass_, y0=yStart, y1=yEnd)
        rows = _lib.params_rows(params)
        torch, device, where, stream = self._target()
        bufs = {name: torch.empty((rows, self.width, ch)[: 3 if ch > 1 else 2],
                                  dtype=torch.float64 if dt is np.float64 else torch.int32, device=where)
                for name, ch, dt in _lib.AOV_BUFFERS}
        if rows > 0:  # an empty row set has no buffers to point at
            scene._device_scene(device).render_aov_async(
                self.Camera._state, params, *(bufs[name].data_ptr() for name, _, _ in _lib.AOV_BUFFERS),
                stream=stream)
        return {name: t.cpu().numpy() for name, t in bufs.items()}

    def _denoise_device(self, torch, colour, aov: dict, overrides: dict):
        """tray_denoise_async on device tensors: colour (rows, W, 3) float64 and the guides of
        `aov` (albedo, normal, depth; a missing or None entry drops its term) -> a new
        (rows, W, 3) float64 tensor, enqueued on the current stream."""
        rows, width = int(colour.shape[0]), int(colour.shape[1])
        params = _lib.denoise_params(width, rows, **overrides)
        nbytes = _lib.denoise_workspace_bytes(params)
        out = torch.empty_like(colour)
        work = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=colour.device)
        _lib.denoise_async(colour.data_ptr(), params, out.data_ptr(), work.data_ptr() if nbytes else None, nbytes,
                           *_guide_ptrs(aov), device=colour.device.index or 0,
                           stream=torch.cuda.current_stream(colour.device).cuda_stream)
        # `work` may be freed here: torch's allocator reuses it only for work on this same stream
        return out

    def _denoise_variance_device(self, torch, colour, variance, aov: dict, overrides: dict):
        """tray_denoise_variance_async on device tensors, as _denoise_device: `variance` is the
        (rows, W, 3) variance of the mean `colour`, overrides fields of tray_denoise_variance_params."""
        rows, width = int(colour.shape[0]), int(colour.shape[1])
        params = _lib.denoise_variance_params(width, rows, **overrides)
        nbytes = _lib.denoise_variance_workspace_bytes(params)
        out = torch.empty_like(colour)
        work = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=colour.device)
        _lib.denoise_variance_async(colour.data_ptr(), variance.data_ptr(), params, out.data_ptr(),
                                    work.data_ptr() if nbytes else None, nbytes, *_guide_ptrs(aov),
                                    device=colour.device.index or 0,
                                    stream=torch.cuda.current_stream(colour.device).cuda_stream)
        return out

    def Denoise(self, frame, aov: dict, yStart: int = 0, yEnd: int | None = None, tile_rows: int = 0,
                **overrides) -> np.ndarray:
        """The guided a-trous filter of include/tray_denoise.h over `frame`, a linear (rows, W, 3)
        float64 image (Tracer.linear), with the feature buffers RenderAOV returned for the same
        rows: (rows, W, 3) float64. overrides: fields of tray_denoise_params (iterations, flags,
        sigma_color, sigma_normal, sigma_depth). No Go counterpart.

        yStart, yEnd and tile_rows change nothing in the result: they exist only so that a caller
        who rendered a row set can say which, and be refused where the filter cannot serve it. The
        filter needs spatially contiguous rows, so [yStart, yEnd) must be a row range of the image
        with exactly the frame's number of rows (else ValueError), and any tile_rows > 0, an
        interleaved row set, raises ValueError."""
        yEnd = self.height if yEnd is None else yEnd
        if tile_rows > 0:
            raise ValueError("Denoise needs spatially contiguous rows: interleaved row sets (tile_rows > 0) are not")
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        if not 0 <= yStart <= yEnd <= self.height or frame.shape != (yEnd - yStart, self.width, 3):
            raise ValueError(f"frame must hold rows [{yStart}, {yEnd}) of the {self.width}-wide image as "
                             f"(rows, W, 3); got {frame.shape}")
        guides = self._upload_guides(aov, frame.shape[0])
        if frame.size == 0:
            _lib.denoise_params(self.width, 0, **overrides)  # still refuses unknown fields
            return frame.copy()
        torch, _, where, _ = self._target()
        return self._denoise_device(torch, torch.from_numpy(frame).to(where), guides, overrides).cpu().numpy()

    def RenderDenoised(self, scene: Scene | None, **overrides) -> np.ndarray:
        """Render(scene) at the tracer's few rays per pixel, made presentable: a linear FP64
        render (tray_render_async), the feature buffers of the same samples
        (tray_render_aov_async), the guided filter (tray_denoise_async) and ColorF.ToSRGBA
        (tray_linear_to_srgba_async), all enqueued on one stream with no host round trip in
        between. Returns (H, W, 4) uint8 RGBA like Render and keeps it in imageData; `linear`
        holds the denoised FP64 frame. overrides as for Denoise."""
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        params = self._params(self._seed())
        if self.height * self.width == 0:
            return self.imageData
        torch, device, where, stream = self._target()
        dev = scene._device_scene(device)
        colour = torch.empty((self.height, self.width, 3), dtype=torch.float64, device=where)
        aov = self._guide_buffers(torch, where)
        dev.render_async(self.Camera._state, params, colour.data_ptr(), None, stream)
        dev.render_aov_async(self.Camera._state, params, *_guide_ptrs(aov), stream=stream)
        return self._show(torch, self._denoise_device(torch, colour, aov, overrides), device, stream)

    def Accumulate(self, frames, tolerance: float | None = None, floor: float | None = None):
        """The running mean of a stack of linear frames, (k, rows, W, 3) float64 (for instance k
        progressive passes of the same pixels), and the per-channel variance of that mean
        (include/tray_progressive.h, sections 1 and 2): two (rows, W, 3) float64 arrays, folded
        on the device in one launch. The variance is +inf for k < 2. `unconverged` and
        `max_ratio` receive the convergence record for `tolerance` and `floor` (the library's
        defaults when None). Any rows of the image's width do. No Go counterpart."""
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        if frames.ndim != 4 or frames.shape[2:] != (self.width, 3) or frames.shape[0] < 1:
            raise ValueError(f"frames must be (k, rows, {self.width}, 3) with k >= 1; got {frames.shape}")
        k, rows = frames.shape[:2]
        mp = _lib.accum_metric_params(**_given(tolerance=tolerance, floor=floor))
        if rows * self.width == 0:
            self.unconverged, self.max_ratio = 0, 0.0
            return frames[0].copy(), frames[0].copy()
        torch, device, where, stream = self._target()
        stack = torch.from_numpy(frames).to(where)
        mean, m2, variance = (torch.empty((rows, self.width, 3), dtype=torch.float64, device=where) for _ in range(3))
        record = torch.empty((2,), dtype=torch.float64, device=where)
        acc = _lib.Accum(mean.data_ptr(), m2.data_ptr(), self.width, rows, 0, 0)
        _lib.accum_fold_metric_async(acc, stack.data_ptr(), k, mp, variance.data_ptr(), record.data_ptr(), device,
                                     stream)
        rec = record.cpu().numpy().view(_lib.ACCUM_METRIC_DTYPE)[0]
        self.unconverged, self.max_ratio = int(rec["unconverged"]), float(rec["max_ratio"])
        return mean.cpu().numpy(), variance.cpu().numpy()

    def RenderProgressive(self, scene: Scene | None, max_passes: int, batch: int = 4, tolerance: float | None = None,
                          denoise: bool = False, guides: dict | None = None, fraction: float = 0.0,
                          floor: float | None = None, **overrides) -> np.ndarray:
        """Keeps rendering until the picture is good enough: progressive passes of
        NumRaysPerPixel samples each (tray_render_passes_async, `batch` passes per launch into one
        device buffer), folded into a running mean with the variance of that mean and the
        convergence record (tray_accum_fold_metric_async), and a 16-byte readback per batch. It
        stops when at most `fraction` of the pixels are unconverged at `tolerance` (the relative
        standard error; the library's default when None; never before 2 passes, whose variance is
        the first there is), or after max_passes. The seed is drawn once for the whole call and
        kept in `seed`, so the passes are one random stream also with Seed = 0. Everything is
        enqueued on one stream and no frame leaves the device before the end.

        With denoise=True the mean goes through the variance-guided filter
        (tray_denoise_variance_async; overrides: fields of tray_denoise_variance_params), guided by
        `guides` (a dict of albedo, normal, depth arrays as RenderAOV returns) or, when None, by the
        feature buffers of the first pass (tray_render_aov_async). Returns (H, W, 4) uint8 RGBA
        (tray_linear_to_srgba_async) like Render and keeps it in imageData; `linear` holds the FP64
        frame shown, `variance` the per-channel variance of the mean, `passes` the passes done,
        `unconverged` and `max_ratio` the last record. No Go counterpart."""
        if max_passes < 1 or batch < 1:
            raise ValueError("max_passes and batch must be >= 1")
        if overrides and not denoise:
            raise ValueError(f"filter parameters {sorted(overrides)} given without denoise=True")
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        self.seed = self._seed()  # once: every pass draws from this stream
        mp = _lib.accum_metric_params(**_given(tolerance=tolerance, floor=floor))
        h, w = self.height, self.width
        self.passes, self.unconverged, self.max_ratio = 0, h * w, 0.0
        self.variance = np.full((h, w, 3), np.inf)
        if h * w == 0:
            return self.imageData
        torch, device, where, stream = self._target()
        dev = scene._device_scene(device)
        f64 = dict(dtype=torch.float64, device=where)
        frames = torch.empty((min(batch, max_passes), h, w, 3), **f64)
        mean, m2, variance = (torch.empty((h, w, 3), **f64) for _ in range(3))
        record = torch.empty((2,), **f64)
        acc = _lib.Accum(mean.data_ptr(), m2.data_ptr(), w, h, 0, 0)
        aov = self._frame_guides(torch, dev, guides, where, stream) if denoise else None
        while self.passes < max_passes:
            n = min(batch, max_passes - self.passes)
            dev.render_passes_async(self.Camera._state, self._params(self.seed, self.passes), n, frames.data_ptr(),
                                    stream)
            _lib.accum_fold_metric_async(acc, frames.data_ptr(), n, mp, variance.data_ptr(), record.data_ptr(),
                                         device, stream)
            rec = record.cpu().numpy().view(_lib.ACCUM_METRIC_DTYPE)[0]  # the 16-byte readback
            self.passes = int(acc.count)
            self.unconverged, self.max_ratio = int(rec["unconverged"]), float(rec["max_ratio"])
            if self.passes >= 2 and self.unconverged <= fraction * (h * w):
                break
        shown = self._denoise_variance_device(torch, mean, variance, aov, overrides) if denoise else mean
        self._show(torch, shown, device, stream)
        self.variance = variance.cpu().numpy()
        return self.imageData

    def RenderPixels(self, scene: Scene | None, pixels, passes: int = 1, pass_: int = 0) -> np.ndarray:
        """The linear FP64 colour of the listed pixels alone (tray_render_pixels_async): `pixels` holds
        n indices y * width + x of the frame Render(scene) draws, with Render's defaulting; returns
        (passes, n, 3) float64, progressive passes pass_ .. pass_ + passes - 1. Each value has the
        bits of that pixel in an ordered-sum render of that pass (TRAY_FLAG_ORDERED_SUM), whichever
        other pixels are listed; an index outside the image gets zeros. For a region of interest or
        for rendering a picked pixel again. Set Seed for values that repeat. No Go counterpart."""
        if passes < 1:
            raise ValueError("passes must be >= 1")
        idx = np.ascontiguousarray(pixels)
        if idx.ndim != 1 or (idx.size and (idx.dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= 2 ** 32)):
            raise ValueError("pixels must be a 1-d array of indices y * width + x in [0, 2^32)")
        idx = idx.astype(np.uint32)
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        params = self._params(self._seed(), pass_)
        torch, device, where, stream = self._target()
        n = int(idx.size)
        out = torch.empty((passes, n, 3), dtype=torch.float64, device=where)
        lst = torch.from_numpy(idx.view(np.int32)).to(where)
        scene._device_scene(device).render_pixels_async(
            self.Camera._state, params, lst.data_ptr() if n else None, n, out.data_ptr() if n else None, passes,
            stream=stream)
        return out.cpu().numpy()

    def RenderAdaptive(self, scene: Scene | None, max_passes: int, min_passes: int | None = None, batch: int = 4,
                       tolerance: float | None = None, floor: float | None = None, dilate: int = 1,
                       denoise: bool = False, guides: dict | None = None, **overrides) -> np.ndarray:
        """RenderProgressive that spends its samples where the picture is still noisy
        (include/tray_adaptive.h). A warm-up of min_passes uniform passes through the megakernel
        (tray_render_passes_async with the ordered sum, folded by tray_accum_fold_async; the
        library's default when None); then rounds of tray_adaptive_select_async (the per-pixel
        metric, widened by one pixel when `dilate`, compacted into a list), a 32-byte readback,
        tray_render_pixels_async over that list (`batch` more passes of each listed pixel, numbered
        from the pixel's own count) and tray_adaptive_fold_async, all on one stream. It stops when no
        pixel is active: every pixel is converged at `tolerance` or has max_passes. A pixel's k-th
        pass is the same whether it is rendered with the whole frame or in a list, so every pixel's
        (mean, m2) is the uniform ordered-sum state after `counts` passes. The seed is drawn once
        and kept in `seed`.

        denoise, guides and overrides as for RenderProgressive. Returns (H, W, 4) uint8 RGBA and
        keeps it in imageData; `linear` holds the FP64 frame shown, `variance` the per-channel
        variance of the mean, `counts` the (H, W) int32 passes of each pixel, `passes` their maximum,
        `pixel_passes` their sum, `unconverged` and `max_ratio` the last record. No Go counterpart."""
        if max_passes < 1 or batch < 1:
            raise ValueError("max_passes and batch must be >= 1")
        if overrides and not denoise:
            raise ValueError(f"filter parameters {sorted(overrides)} given without denoise=True")
        ap = _lib.adaptive_params(max_passes=int(max_passes), dilate=int(dilate),
                                  **_given(tolerance=tolerance, floor=floor))
        ap.min_passes = min(int(min_passes) if min_passes is not None else ap.min_passes, int(max_passes))
        if ap.min_passes < 1:
            raise ValueError("min_passes must be >= 1")
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        self.seed = self._seed()  # once: every pass draws from this stream
        h, w = self.height, self.width
        self.passes, self.pixel_passes, self.unconverged, self.max_ratio = 0, 0, h * w, 0.0
        self.variance = np.full((h, w, 3), np.inf)
        self.counts = np.zeros((h, w), dtype=np.int32)
        if h * w == 0:
            return self.imageData
        torch, device, where, stream = self._target()
        dev = scene._device_scene(device)
        f64 = dict(dtype=torch.float64, device=where)
        mean, m2, variance = (torch.empty((h, w, 3), **f64) for _ in range(3))
        counts = torch.full((h, w), ap.min_passes, dtype=torch.int32, device=where)
        aov = self._frame_guides(torch, dev, guides, where, stream) if denoise else None
        # The warm-up: uniform passes through the megakernel, in launches of at most `batch`.
        frames = torch.empty((min(batch, ap.min_passes), h, w, 3), **f64)
        acc = _lib.Accum(mean.data_ptr(), m2.data_ptr(), w, h, 0, 0)
        while acc.count < ap.min_passes:
            n = min(batch, ap.min_passes - acc.count)
            dev.render_passes_async(self.Camera._state, self._params(self.seed, acc.count, _lib.FLAG_ORDERED_SUM), n,
                                    frames.data_ptr(), stream)
            _lib.accum_fold_async(acc, frames.data_ptr(), n, device, stream)
        del frames
        state = _lib.AdaptiveState(mean.data_ptr(), m2.data_ptr(), counts.data_ptr(), w, h)
        nbytes = _lib.adaptive_workspace_bytes(w, h)
        work = torch.empty((nbytes // 8,), **f64)
        active = torch.empty((h * w,), dtype=torch.int32, device=where)
        record = torch.empty((4,), **f64)
        values = None

        def select():
            _lib.adaptive_select_async(state, ap, active.data_ptr(), record.data_ptr(), work.data_ptr(), nbytes,
                                       variance.data_ptr(), device, stream)
            return record.cpu().numpy().view(_lib.ADAPTIVE_RECORD_DTYPE)[0]  # the 32-byte readback

        while True:
            rec = select()
            n_active = int(rec["n_active"])
            if n_active == 0:
                break
            if values is None or values.shape[1] < n_active:  # the lists only shrink between rounds, almost
                values = torch.empty((batch, n_active, 3), **f64)
            dev.render_pixels_async(self.Camera._state, self._params(self.seed), active.data_ptr(), n_active,
                                    values.data_ptr(), batch, pass_plane_ptr=counts.data_ptr(), stream=stream)
            _lib.adaptive_fold_async(state, active.data_ptr(), n_active, values.data_ptr(), batch, device, stream)
        self.unconverged, self.max_ratio = int(rec["unconverged"]), float(rec["max_ratio"])
        self.pixel_passes = int(rec["pixel_passes"])
        shown = self._denoise_variance_device(torch, mean, variance, aov, overrides) if denoise else mean
        self._show(torch, shown, device, stream)
        self.variance = variance.cpu().numpy()
        self.counts = counts.cpu().numpy()
        self.passes = int(self.counts.max())
        return self.imageData

    def RenderSequence(self, scene: Scene | None, cameras, denoise: bool = False, variance: bool = False,
                       refill: int = 0, refill_tolerance: float = 1e150, refill_dilate: int = 1,
                       **overrides) -> list:
        """A moving camera that keeps what it has seen (include/tray_temporal.h): frame k is rendered
        through cameras[k] (a sequence of Camera objects, each initialized here for the tracer's size
        as Render does) as progressive pass k of the tracer's one seed, so a still camera sees
        independent samples, and tray_temporal_step_async reprojects the accumulated history of
        frame k - 1 into it and folds the new frame in. The render, the step, with denoise=True the
        guided filter (tray_denoise_async on the feature buffers of the current camera,
        tray_render_aov_async) and the sRGB encoding are enqueued on one stream over two ping-pong
        states; nothing is read back before the last frame is enqueued.

        variance=True (include/tray_temporal_variance.h) runs tray_temporal_var_step_async instead:
        the states carry M2, the colour, ages and records are the same bits, `variance` keeps the
        last frame's (H, W, 3) variance of the mean and `m2` its M2, and denoise=True then means the
        variance-guided filter (tray_denoise_variance_async on the step's variance) in place of the
        plain one, which damages a pixel that holds many samples. With either filter `filtered`
        keeps the last frame as shown, (H, W, 3) FP64, before the sRGB encoding.

        refill=R > 0 implies variance=True and spends R more passes per frame on the pixels that
        hold fewer than 1 + R frames (the fresh ones: disocclusions, the frame's leading edge and all
        of frame 0) and, with refill_dilate 1, on their 8 neighbours: tray_adaptive_select_async on
        the state as a tray_adaptive_state (min_passes 1 + R, max_passes max_history), a 32-byte
        readback of its record for the list's length, tray_render_pixels_async,
        tray_adaptive_fold_async and tray_temporal_var_variance_async over the list. Frame k then
        owns the progressive passes k (1 + R) .. (k + 1)(1 + R) - 1: the uniform frame is the
        first, the refill the rest, so no sample repeats. refill_tolerance is the selection's
        tolerance; at the default 1e150 only the count decides. A real tolerance (0.05, say)
        refills by variance, which selects most of an r = 4 frame: a list renderer breaks even with
        the whole-frame renderer at an active fraction of about 0.18, so that is
        rarely worth it. `refilled` holds the per-frame list lengths, `pixel_passes` the passes
        spent in all (H x W per frame plus R per listed pixel); `age` and `linear` include the refill,
        `fresh` and `mean_age` are the step's records, before it.

        overrides: fields of tray_temporal_params (max_history, depth_tolerance, snap, flags).
        Returns the list of (H, W, 4) uint8 RGBA frames and keeps the last in imageData; `linear`
        holds the last accumulated FP64 frame (before the filter), `age` its (H, W) int32 ages, `fresh`
        and `mean_age` the per-frame lists from the records (fresh pixels; the mean output age).
        ValueError for an empty sequence, an entry that is not a Camera, an unknown override, a
        refill that is not an integer >= 0 or exceeds max_history - 1 (a pixel could never hold
        1 + R frames), a refill_tolerance that is not finite, >= 0 and of finite square, or a
        refill_dilate other than 0 or 1, before any device work. No Go counterpart."""
        refill, rt = _refill_options(refill, refill_tolerance, refill_dilate)
        variance = bool(variance) or refill > 0
        cameras = list(cameras) if cameras is not None else []
        if not cameras:
            raise ValueError("cameras must hold at least one Camera")
        if not all(isinstance(c, Camera) for c in cameras):
            raise ValueError("cameras must be a sequence of Camera objects")
        tp = _temporal_options(overrides, refill)
        scene = self._apply_defaults(scene)
        h, w = self.height, self.width
        for c in cameras:
            c.Initialize(w, h)
        object.__setattr__(self, "Camera", cameras[-1])
        self.seed = self._seed()  # once: every frame is a pass of this stream
        self._reset_temporal_fields(variance)
        if h * w == 0:
            return [self.imageData.copy() for _ in cameras]
        torch, device, where, stream = self._target()
        dev = scene._device_scene(device)
        loop = _TemporalLoop(self, torch, device, where, stream, len(cameras), tp, variance, refill, rt,
                             refill_dilate, denoise)
        for k, cam in enumerate(cameras):
            loop.frame(k, dev, cam, cameras[k - 1] if k else None)
        return loop.finish()

    def _reset_temporal_fields(self, variance: bool) -> None:
        """What _TemporalLoop.finish() sets, as an empty image leaves it."""
        h, w = self.height, self.width
        self.age = np.zeros((h, w), dtype=np.int32)
        self.fresh, self.mean_age = [], []
        if variance:
            self.variance = np.full((h, w, 3), np.inf)
            self.m2 = np.zeros((h, w, 3))
            self.refilled, self.pixel_passes = [], 0

    def RenderAnimation(self, scene: Scene | None, geometries, denoise: bool = False, temporal: bool = False,
                        variance: bool = False, refill: int = 0, refill_tolerance: float = 1e150,
                        refill_dilate: int = 1, cameras=None, **overrides) -> list:
        """Moving spheres under the tracer's camera (include/tray_scene_update.h): frame k shows the
        scene with its spheres at geometries[k], a (k, n, 4) float64 array or device tensor of
        {cx, cy, cz, radius} per sphere in list order, as progressive pass k of the tracer's one
        seed. The scene is uploaded once; each frame is tray_scene_update_async, tray_render_async,
        with denoise=True the feature buffers and the guided filter (tray_render_aov_async,
        tray_denoise_async), and the sRGB encoding, all enqueued on one stream; nothing is read back
        before the last frame is enqueued. A device tensor is used where it is: no copy to the host.

        `applied` lists each frame's record: 1 where the spheres were moved in place, 0 where the
        update was refused (a sphere left the bound of the scene as uploaded, section 2 of the
        header). The records are read with the frames, so a refusal is found late: that frame is
        then made by a release and a fresh upload of its geometry, and the frames after it again by
        updates of the new copy. Every frame has the bits of a fresh upload's render either way.

        temporal=True (include/tray_temporal_motion.h) keeps what the frames before have seen: frame k
        is update, render, tray_temporal_motion_step_async with geometries[k - 1] as the previous
        geometry (the tensor where it is), the optional refill chain, the optional filter and the
        encoding, on one stream over two ping-pong states: the history follows each hit point with
        its sphere. variance, refill, refill_tolerance, refill_dilate and the overrides (fields of
        tray_temporal_params) mean what they mean in RenderSequence, and `age`, `fresh`, `mean_age`,
        `variance`, `m2`, `refilled`, `pixel_passes` and `filtered` are set as there; `linear` is the
        last accumulated frame. The 32-byte update record of frame k is then read before frame k is
        rendered (one small readback per frame, as the refill chain has): on a refusal the scene is
        released and uploaded afresh with geometries[k] at once, and the history carries over
        unchanged, since the step takes the previous geometry as a buffer and sphere order is the
        list order either way. History follows surfaces, not light: what a moved neighbour changes
        in a static surface's shading arrives with the lag of max_history (the header, section 5).

        cameras: an optional sequence of k Cameras, frame k through cameras[k] (each initialized
        here); the tracer's camera for every frame by default. Without temporal they only replace
        the camera per frame.

        Returns the list of (H, W, 4) uint8 RGBA frames and keeps the last in imageData and, before
        the encoding, in `linear`; the scene's Objects end at the last geometry. ValueError for an
        empty sequence or a shape other than (k, n, 4), for cameras whose length is not k or that
        hold anything but Cameras, for variance, refill, their two options or an override without
        temporal=True, and with it for what RenderSequence refuses, before any device work. No Go
        counterpart."""
        if not temporal and (variance or refill or overrides or refill_tolerance != 1e150 or refill_dilate != 1):
            raise ValueError("variance, refill, refill_tolerance, refill_dilate and temporal parameters need "
                             "temporal=True")
        if temporal:
            refill, rt = _refill_options(refill, refill_tolerance, refill_dilate)
            variance = bool(variance) or refill > 0
            tp = _temporal_options(overrides, refill)
        if cameras is not None:
            cameras = list(cameras)
            if not all(isinstance(c, Camera) for c in cameras):
                raise ValueError("cameras must be a sequence of Camera objects")
        scene = self._apply_defaults(scene)
        self.Camera.Initialize(self.width, self.height)
        import torch

        n, h, w = len(scene.Objects), self.height, self.width
        on_device = torch.is_tensor(geometries)
        if not on_device:
            geometries = np.ascontiguousarray(geometries, dtype=np.float64)
        if geometries.ndim != 3 or tuple(geometries.shape[1:]) != (n, 4) or geometries.shape[0] < 1:
            raise ValueError(f"geometries must be (k, {n}, 4) with k >= 1; got {tuple(geometries.shape)}")
        if on_device and geometries.dtype != torch.float64:
            raise ValueError("geometries must be float64")
        count = int(geometries.shape[0])
        if cameras is not None:
            if len(cameras) != count:
                raise ValueError(f"cameras must hold one Camera per frame ({count}); got {len(cameras)}")
            for c in cameras:
                c.Initialize(w, h)
            object.__setattr__(self, "Camera", cameras[-1])
        else:
            cameras = [self.Camera] * count
        self.seed = self._seed()  # once: every frame is a pass of this stream
        self.applied = []
        if temporal:
            self._reset_temporal_fields(variance)
        if h * w == 0:
            return [self.imageData.copy() for _ in range(count)]
        torch, device, where, stream = self._target()
        geo = geometries.to(where).contiguous() if on_device else torch.from_numpy(geometries).to(where)
        dev = scene._device_scene(device)
        if temporal:
            loop = _TemporalLoop(self, torch, device, where, stream, count, tp, variance, refill, rt, refill_dilate,
                                 denoise)
            record = torch.zeros((_lib.SCENE_UPDATE_RECORD_DTYPE.itemsize // 8,), dtype=torch.float64, device=where)
            for k in range(count):
                applied = 1
                if n:
                    dev.update_async(geo[k].data_ptr(), n, record.data_ptr(), stream)
                    applied = int(record.cpu().numpy().view(_lib.SCENE_UPDATE_RECORD_DTYPE)[0]["applied"])  # 32 bytes
                    if not applied:  # refused: this geometry as a fresh upload; the history stays
                        scene._set_geometry(geo[k].cpu().numpy())
                        dev.release()
                        scene._adopt(device, None)
                        dev = scene._device_scene(device)
                self.applied.append(applied)
                loop.frame(k, dev, cameras[k], cameras[k - 1] if k else None,
                           (geo[k - 1].data_ptr() if k and n else None, n))
            scene._set_geometry(geo[count - 1].cpu().numpy())
            scene._adopt(device, dev)
            return loop.finish()
        records = torch.zeros((count, _lib.SCENE_UPDATE_RECORD_DTYPE.itemsize // 8), dtype=torch.float64, device=where)
        rgba = torch.empty((count, h, w, 4), dtype=torch.uint8, device=where)
        colour = torch.empty((h, w, 3), dtype=torch.float64, device=where)
        aov = self._guide_buffers(torch, where) if denoise else None
        start, uploaded = 0, False  # uploaded: frame `start` is the geometry of a fresh upload
        while start < count:
            for k in range(start, count):
                if n and not (uploaded and k == start):
                    dev.update_async(geo[k].data_ptr(), n, records[k].data_ptr(), stream)
                params = self._params(self.seed, k)
                dev.render_async(cameras[k]._state, params, colour.data_ptr(), None, stream)
                shown = colour
                if denoise:
                    dev.render_aov_async(cameras[k]._state, params, *_guide_ptrs(aov), stream=stream)
                    shown = self._denoise_device(torch, colour, aov, {})
                _lib.linear_to_srgba_async(shown.data_ptr(), h * w, rgba[k].data_ptr(), device, stream)
            flags = records.cpu().numpy().reshape(-1).view(_lib.SCENE_UPDATE_RECORD_DTYPE)["applied"]
            flags = [1 if n == 0 else int(f) for f in flags[start:]]
            if uploaded:
                flags[0] = 0
            refused = [i for i, f in enumerate(flags) if not f and not (uploaded and i == 0)]
            good = refused[0] if refused else len(flags)
            self.applied += flags[:good]
            if not refused:
                break
            start, uploaded = start + good, True  # this frame and the ones after it: again, from a fresh upload
            scene._set_geometry(geo[start].cpu().numpy())
            dev.release()
            scene._adopt(device, None)
            dev = scene._device_scene(device)
        self.linear[:] = shown.cpu().numpy()
        scene._set_geometry(geo[count - 1].cpu().numpy())
        scene._adopt(device, dev)
        frames = [f.copy() for f in rgba.cpu().numpy()]
        self.imageData[:] = frames[-1]
        return frames

    def RenderLines(self, idx: int, yStart: int, yEnd: int, scene: Scene) -> None:  # ray/tracer.go:120-155
        """Render rows [yStart, yEnd) with the current (initialized) camera and
        fields; like Go, no defaulting happens here."""
        if self.Camera._state is None:
            raise _lib.TrayError(_lib.TRAY_ERR_INVALID_ARGUMENT, "Camera.Initialize must be called first")
        self._render_rows(yStart, yEnd, scene)


def New(width: int, height: int) -> Tracer:  # ray/tracer.go:38-45
    return Tracer(width, height)
