"""Frame recording without a GPU: the shapes header through its host twin against the float64 reference, the PNG writer, the binding, the
command-line flags of both trees, and the reference's own edge-pixel share on the scenes the GPU tests use."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi
from tests import render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
GRAZING = 0.05          # |n.d| below this is a grazing hit: its t is not compared (the discriminant's square root amplifies without bound)


def t_tolerance(S, g):
    """|t_fp32 - t_float64| for a hit at distance scale S (origin to primitive) and incidence cosine g.  The header takes the discriminant as
    r^2 - |p|^2 with p = oc - (oc.d) d; p carries ~3 roundings of size eps S, so the discriminant is off by <= 2 |p| 3 eps S <= 6 r eps S, and
    its square root (= r g at the hit) by <= 3 eps S / g; -(oc.d) adds ~3 eps S and the inputs' own normalisation error eps S.  The box's
    slab quotient (h - ol) / dl has the same shape: ol is off by ~3 eps S and dl = g.  Doubled for the capsule's extra projection:
    16 eps S (1 + 1 / g)."""
    return 16.0 * EPS32 * S * (1.0 + 1.0 / g)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("rshapes")
    so = str(d / "libqa_render_shapes_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "c_host", "qa_render_shapes_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.qa_render_shapes_host.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3; lib.qa_render_shapes_host.restype = C.c_int
    lib.qa_render_shapes_table_host.argtypes = [C.c_void_p, C.c_int]; lib.qa_render_shapes_table_host.restype = C.c_int
    return lib


def _table(lib_fn):
    buf = np.zeros((64, 10), np.float32)
    n = lib_fn(buf.ctypes.data, 64)
    return [dict(kind=int(r[0]), body=int(r[1]), cls=int(r[2]), a=tuple(float(v) for v in r[3:6]), b=tuple(float(v) for v in r[6:9]), r=float(r[9]))
            for r in buf[:n]]


def _rand_rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return rr.quat_matrix(q)


def _unit32(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def _cases(kind, rng, n=300):
    """rays (n,6) and primitives (n,16) in fp32: random poses and sizes of the robot's range, rays aimed at or just past the primitive, plus
    the special families (axis-parallel rays for the box, rays along the axis for the capsule)"""
    rays, prims = np.zeros((n, 6), np.float32), np.zeros((n, 16), np.float32)
    for i in range(n):
        c = rng.uniform(-2, 2, 3)
        R = _rand_rot(rng)
        r = rng.uniform(0.01, 0.2)
        special = i % 5 == 4
        if kind == rr.SPHERE:
            a, b, reach = c, np.zeros(3), r
        elif kind == rr.CAPSULE:
            if special:
                R = np.eye(3)[:, rng.permutation(3)]
            hl = rng.uniform(0.02, 0.15)
            a, b, reach = c - hl * R[:, 0], c + hl * R[:, 0], hl + r
        else:
            if special:
                R = np.eye(3)[:, rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)
            a, b = c, rng.uniform(0.01, 0.2, 3)
            reach = float(np.linalg.norm(b)); r = 0.0
        o = c + rng.uniform(0.5, 5.0) * _unit32(rng.normal(size=3)).astype(np.float64)
        if special and kind == rr.CAPSULE:                       # along the axis, inside or outside the radius
            off = R[:, 1] * rng.uniform(0, 1.5) * r
            sgn = rng.choice([-1.0, 1.0])
            o = c + off - sgn * rng.uniform(0.5, 3.0) * R[:, 0]
            d = sgn * R[:, 0]
        elif special and kind == rr.BOX:                         # parallel to a world axis = to one of the box's axes: exact zeros in dl
            ax = int(rng.integers(3)); sgn = rng.choice([-1.0, 1.0])
            d = np.zeros(3); d[ax] = sgn
            lat = R @ (rng.uniform(-1.3, 1.3, 3) * b)
            o = c + lat - d * ((lat @ d) + rng.uniform(0.5, 3.0))
        else:
            tgt = c + rng.uniform(0, 1.25) * reach * _unit32(rng.normal(size=3)).astype(np.float64)
            d = tgt - o
        rays[i, :3], rays[i, 3:] = o, _unit32(d)
        prims[i, :3], prims[i, 3:6], prims[i, 6], prims[i, 7:] = a, b, r, R.ravel()
    return rays, prims


def _ref(kind, ray, prim, d=None):
    o = ray[:3].astype(np.float64); d = ray[3:].astype(np.float64) if d is None else d
    p = prim.astype(np.float64)
    if kind == rr.SPHERE:
        t, n = rr.ray_sphere(o, d, p[:3], p[6])
    elif kind == rr.CAPSULE:
        t, n = rr.ray_capsule(o, d, p[:3], p[3:6], p[6])
    else:
        t, n = rr.ray_box(o, d, p[:3], p[7:].reshape(3, 3), p[3:6])
    return float(t[0]), n[0]


@pytest.mark.parametrize("kind", [rr.SPHERE, rr.CAPSULE, rr.BOX])
def test_header_intersections_match_the_float64_reference(twin, kind):
    rng = np.random.default_rng(10 + kind)
    rays, prims = _cases(kind, rng)
    out = np.zeros((rays.shape[0], 5), np.float32)
    assert twin.qa_render_shapes_host(kind, rays.shape[0], rays.ctypes.data, prims.ctypes.data, out.ctypes.data) == 0
    compared = hits = 0
    worst_t = worst_n = 0.0
    for i in range(rays.shape[0]):
        t, n = _ref(kind, rays[i], prims[i])
        d = rays[i, 3:].astype(np.float64)
        # away from edges: the four rays turned by 1e-4 rad agree with the centre ray on hit / miss
        e1 = np.cross(d, [1.0, 0, 0] if abs(d[0]) < 0.9 else [0, 1.0, 0]); e1 /= np.linalg.norm(e1); e2 = np.cross(d, e1)
        same = all(np.isfinite(_ref(kind, rays[i], prims[i], (d + s * e) / np.linalg.norm(d + s * e))[0]) == np.isfinite(t)
                   for e in (e1, e2) for s in (1e-4, -1e-4))
        if not same:
            continue
        compared += 1
        assert bool(out[i, 0]) == bool(np.isfinite(t)), (i, out[i], t)
        if not np.isfinite(t):
            continue
        g = abs(float(n @ d))
        if g < GRAZING:
            continue
        hits += 1
        S = float(np.linalg.norm(rays[i, :3].astype(np.float64) - prims[i, :3])) + 0.5
        tol = t_tolerance(S, g)
        worst_t = max(worst_t, abs(float(out[i, 1]) - t) / tol)
        assert abs(float(out[i, 1]) - t) <= tol, (i, out[i, 1], t, tol)
        r = float(prims[i, 6])
        tol_n = 1e-6 + ((tol + 4 * EPS32 * S) / r if kind != rr.BOX else 0.0)     # a curved normal is (hit point - centre) / r
        worst_n = max(worst_n, float(np.abs(out[i, 2:] - n).max()) / tol_n)
        assert np.abs(out[i, 2:] - n).max() <= tol_n, (i, out[i, 2:], n, tol_n)
    print(f"kind {kind}: {compared} rays compared, {hits} hits; worst |dt| / tol {worst_t:.3f}, worst |dn| / tol {worst_n:.3f}")
    assert compared > 200 and hits > 80


def test_rays_starting_inside_report_no_hit(twin):
    rays = np.zeros((3, 6), np.float32); rays[:, 3] = 1.0
    prims = np.zeros((3, 16), np.float32)
    prims[0, 6] = 0.1
    prims[1, :3], prims[1, 3:6], prims[1, 6] = (-0.2, 0, 0), (0.2, 0, 0), 0.05
    prims[2, 3:6], prims[2, 7:] = (0.1, 0.1, 0.1), np.eye(3).ravel()
    for kind in (rr.SPHERE, rr.CAPSULE, rr.BOX):
        out = np.ones((1, 5), np.float32)
        twin.qa_render_shapes_host(kind, 1, rays[kind].ctypes.data, prims[kind].ctypes.data, out.ctypes.data)
        assert out[0, 0] == 0.0
        assert not np.isfinite(_ref(kind, rays[kind], prims[kind])[0])


def test_table_is_the_same_on_host_twin_and_library_and_covers_every_body(twin):
    import __graft_entry__ as g
    g.build()
    lib = _capi.load_library()
    host, built = _table(twin.qa_render_shapes_table_host), _table(lib.qa_render_shape_table)
    assert host == built and len(host) == 23
    assert sorted({p["body"] for p in host}) == list(range(19))
    names = _capi.BODY_NAMES
    for p in host:
        want = {"hip": 1, "thigh": 2, "calf": 3, "foot": 4}.get(names[p["body"]].split("_")[-1], 0)
        assert p["cls"] == want, (p, names[p["body"]])
    # left hips sit at +y, right hips at -y (the URDF's hip collision origins)
    for leg, sy in enumerate((1, -1, 1, -1)):
        hip = [p for p in host if p["body"] == 3 + 4 * leg][0]
        assert hip["kind"] == rr.CAPSULE and np.sign(hip["a"][1]) == sy and abs(0.5 * (hip["a"][1] + hip["b"][1])) == pytest.approx(0.08)


# ------------------------------------------------------------------ PNG
def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body)); pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, inter) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()                       # filter type 0 on every scanline: nothing to undo
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trips(tmp_path):
    from quadrupedal_agility_amd.render import write_png
    a = np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    path = write_png(str(tmp_path / "sub" / "7.png"), a)
    got = _decode_png(open(path, "rb").read())
    assert got.shape == (37, 53, 3) and np.array_equal(got, a)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), a.astype(np.float32))


# ------------------------------------------------------------------ binding
def test_library_exports_the_entry_point_and_capi_mirrors_the_header():
    import __graft_entry__ as g
    g.build()
    assert ("qa_render.hip", []) in g.HIP_SOURCES and "qa_render_shapes.h" in g.HIP_HEADERS
    assert os.path.join(ROOT, "include", "qa_render.h") in g._lib_sources()
    lib = _capi.load_library()
    assert "render_frames" in _capi.EXTENSION_SYMBOLS and "render_frames" not in _capi.ABI_SYMBOLS
    f = lib.qa_render_frames
    assert f.restype == C.c_int and len(f.argtypes) == 3
    assert C.sizeof(_capi.QaRenderCfg) == lib.qa_render_sizeof(0) == 15 * 4
    assert C.sizeof(_capi.QaRenderIo) == lib.qa_render_sizeof(1) == 9 * 8
    text = open(os.path.join(ROOT, "include", "qa_render.h")).read()
    for name in [n for n, _ in _capi.QaRenderCfg._fields_] + list(_capi.RENDER_IO_FIELDS):
        assert name in text, name
    assert f(None, None, None) == -1                                                   # QA_E_ARG (nothing touches the device)
    cfg, io = _capi.QaRenderCfg(), _capi.QaRenderIo()
    cfg.num_envs, cfg.num_cameras, cfg.width, cfg.height, cfg.far = 4, 0, 64, 48, 10.0
    cfg.light_dir[2] = 1.0
    assert f(C.byref(cfg), C.byref(io), None) == -1 and b"num_cameras" in lib.qa_last_error()      # K = 0
    cfg.num_cameras = 1
    assert f(C.byref(cfg), C.byref(io), None) == -1 and b"required" in lib.qa_last_error()         # NULL rgb / body_state
    assert len(__import__("quadrupedal_agility_amd.render", fromlist=["palette"]).palette(lib)) == 8


# ------------------------------------------------------------------ flags and config
def test_record_flags_reach_the_play_configuration_in_both_trees(tmp_path):
    from quadrupedal_agility_amd.legged_gym.utils import helpers as bbc
    from quadrupedal_agility_amd.tsc.legged_gym.utils import helpers as tsc
    from quadrupedal_agility_amd.render import record_settings
    for h in (bbc, tsc):
        a = h.get_args(["--record_frames", str(tmp_path), "--record_envs", "0,3", "--record_every", "3", "--frame_size", "64x48"])
        assert record_settings(a, "exp") == dict(out_dir=str(tmp_path), env_ids=(0, 3), size=(64, 48), every=3)
        a = h.get_args(["--record_frames"])
        assert record_settings(a, "exp") == dict(out_dir=os.path.join("logs", "exp", "exported", "frames"), env_ids=(0,), size=(640, 360), every=2)
        assert record_settings(h.get_args([]), "exp") is None
        a = h.get_args(["--record_frames", "--record_offset", "0,-1.2,2.6"])
        assert record_settings(a, "exp")["offset"] == (0.0, -1.2, 2.6) and record_settings(h.get_args(["--record_frames"]), "exp", (1.0, 2.0, 3.0))["offset"] == (1.0, 2.0, 3.0)
        with pytest.raises(ValueError):
            record_settings(h.get_args(["--record_frames", "--frame_size", "big"]), "exp")


def test_make_qa_config_passes_export_body_state_and_defaults_to_zero():
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    from quadrupedal_agility_amd.legged_gym.utils import helpers
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import make_qa_config
    cfg = Go2LocomotionCfg(); cfg.terrain.mesh_type = "plane"
    assert not hasattr(cfg.sim.qa, "export_body_state")
    assert make_qa_config(cfg).export_body_state == 0
    try:
        helpers.update_cfg_from_args(cfg, None, helpers.get_args(["--record_frames"]))
        assert make_qa_config(cfg).export_body_state == 1
    finally:
        del cfg.sim.qa.export_body_state
    assert make_qa_config(cfg).export_body_state == 0


# ------------------------------------------------------------------ the reference alone: its edge share on the scenes the GPU tests use
def test_reference_flags_few_edge_pixels_on_every_scene():
    from tests.render_scenes import cpu_scenes
    import __graft_entry__ as g
    g.build()
    for name, scene in cpu_scenes().items():
        for k in range(len(scene["env_ids"])):
            ids, depth, rgb, edge = rr.render(scene, k)
            share = float(edge.mean())
            print(f"{name} camera {k}: edge share {share:.4%}, ids {sorted(set(ids.ravel().tolist()))}")
            assert share <= 0.005, (name, k, share)
            assert (ids >= 0).any()                          # something is in view
            # the poses are also chosen so that no pixel's ray meets the ground ON a line of the 0.5 m checker: the two squares differ by
            # 20 % in colour, and a hit point carries ~10 fp32 roundings of coordinates up to 20 m (1.2e-5 m)
            o, d = rr.camera_rays(scene["cameras"][k], scene["width"], scene["height"])
            hp = (o + depth.ravel()[:, None] * d)[ids.ravel() == rr.ID_GROUND, :2] / rr.CHECKER_SIZE
            assert hp.size == 0 or (np.abs(hp - np.round(hp)).min() * rr.CHECKER_SIZE > 2e-5), (name, k)
