"""Independent numpy (float64) ray caster of the rendered scene, written from DESIGN.md §7.1 (tests only).

It is the yardstick of the kernel source (tests/renderhost, host build) and of the HIP kernel: same scene, camera,
shading and pixel conventions, computed in fp64 in world-relative coordinates with its own geometry code (quaternion
rotations, a plain quadratic for the cylinders).  `render()` also returns an `ambiguous` mask: pixels whose segmentation,
shadow state or checker cell changes when the ray moves by +-0.01 pixel, where fp32 and fp64 may legitimately disagree.
"""
import numpy as np

DEFAULT_CAMERA = dict(width=800, height=800, fovy=45.0, distance=1.25, azimuth=45.0, elevation=-25.0)
EXTENT = 0.8
ZNEAR, ZFAR = 0.01 * EXTENT, 50 * EXTENT
FLOOR_Z = -0.02
TORSO_HALF, TORSO_POS = np.array([0.05, 0.0185, 0.0855]), np.array([0.0, 0.0, 0.0995])
WHEEL_R, WHEEL_HL = 0.034, 0.013
WHEEL_POS = (np.array([-0.074, 0.0, 0.034]), np.array([0.074, 0.0, 0.034]))
WHEEL_AXIS_SIGN = (-1.0, 1.0)  # hinge axes: left -x, right +x
BLOCK_HALF = 0.02
CELL, SECTORS = 0.1, 8
FLOOR_RGB = (np.array([0.2, 0.3, 0.4]), np.array([0.1, 0.2, 0.3]))
WHEEL_RGB = (np.array([0.0, 0.0, 0.0]), np.array([0.2, 0.2, 0.2]))
TORSO_RGB, BLOCK_RGB = np.array([0.5, 0.5, 0.5]), np.array([1.0, 0.0, 0.0])
TO_LIGHT = np.array([0.5, 0.5, 1.0]) / np.linalg.norm([0.5, 0.5, 1.0])  # light direction (-0.5, -0.5, -1), reversed
SEG_BG, SEG_FLOOR, SEG_TORSO, SEG_WHEEL_L, SEG_WHEEL_R, SEG_BLOCK = range(6)


def has_block(variant):
    return variant in (2, 3)  # Env03-v1, Env03-v2


def cam_of(camera=None):
    c = dict(DEFAULT_CAMERA)
    c.update(camera or {})
    return c


def camera_frame(camera=None):
    """-> forward, up, right, camera position relative to lookat, tan(fovy / 2) (MuJoCo's free camera)"""
    c = cam_of(camera)
    a, e = np.radians(c["azimuth"]), np.radians(c["elevation"])
    fwd = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    up = np.array([-np.sin(e) * np.cos(a), -np.sin(e) * np.sin(a), np.cos(e)])
    right = np.cross(fwd, up)
    return fwd, up, right, -c["distance"] * fwd, np.tan(np.radians(c["fovy"]) / 2)


def project(point_rel, camera=None):
    """image coordinates (column, row; continuous, pixel centres at i + 1/2) of a point given relative to lookat"""
    c = cam_of(camera)
    fwd, up, right, pos, th = camera_frame(c)
    v = np.asarray(point_rel, float) - pos
    x, y = v @ right / (v @ fwd), v @ up / (v @ fwd)
    W, H = c["width"], c["height"]
    return (x / (th * W / H) + 1) * W / 2, (1 - y / th) * H / 2


def qrot(q, v):
    """rotate vectors v[..., 3] by the unit quaternion q (w, x, y, z)"""
    w, u = q[0], np.asarray(q[1:])
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def qinv(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def scene(qpos, block):
    """moving geoms, lookat-relative: list of (seg id, kind, centre, quaternion, size)"""
    qpos = np.asarray(qpos, float)
    L = qpos[0:3]
    qb = qpos[3:7] / np.linalg.norm(qpos[3:7])
    g = [(SEG_TORSO, "box", qrot(qb, TORSO_POS), qb, TORSO_HALF),
         (SEG_WHEEL_L, "cyl", qrot(qb, WHEEL_POS[0]), qb, None),
         (SEG_WHEEL_R, "cyl", qrot(qb, WHEEL_POS[1]), qb, None)]
    if block:
        qk = qpos[12:16] / np.linalg.norm(qpos[12:16])
        g.append((SEG_BLOCK, "box", qpos[9:12] - L, qk, np.full(3, BLOCK_HALF)))
    return L, qb, g


def interval(kind, centre, q, size, o, d):
    """entry / exit parameters and entry normal (world) of rays o + t d (o, d: [M, 3]) with one convex geom"""
    qi = qinv(q)
    ol, dl = qrot(qi, o - centre), qrot(qi, np.broadcast_to(d, o.shape))
    M = ol.shape[0]
    t_in, t_out = np.full(M, -np.inf), np.full(M, np.inf)
    n = np.zeros((M, 3))

    def slab(k, h):
        nonlocal t_in, t_out
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (-h - ol[:, k]) / dl[:, k], (h - ol[:, k]) / dl[:, k]
        par = dl[:, k] == 0
        lo = np.where(par, np.where(np.abs(ol[:, k]) <= h, -np.inf, np.inf), np.minimum(t1, t2))
        hi = np.where(par, np.where(np.abs(ol[:, k]) <= h, np.inf, -np.inf), np.maximum(t1, t2))
        better = lo > t_in
        e = np.zeros(3); e[k] = 1
        n[better] = -np.sign(dl[better, k])[:, None] * e
        t_in, t_out = np.where(better, lo, t_in), np.minimum(t_out, hi)

    if kind == "box":
        for k in range(3):
            slab(k, size[k])
    else:  # cylinder along local x
        slab(0, WHEEL_HL)
        a = dl[:, 1] ** 2 + dl[:, 2] ** 2
        b = ol[:, 1] * dl[:, 1] + ol[:, 2] * dl[:, 2]
        c = ol[:, 1] ** 2 + ol[:, 2] ** 2 - WHEEL_R ** 2
        disc = b * b - a * c
        ok = (a > 0) & (disc >= 0)
        sq = np.sqrt(np.where(ok, disc, 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.where(ok, (-b - sq) / a, np.where((a == 0) & (c <= 0), -np.inf, np.inf))
            hi = np.where(ok, (-b + sq) / a, np.where((a == 0) & (c <= 0), np.inf, -np.inf))
        better = lo > t_in
        pl = ol + np.where(np.isfinite(lo), lo, 0)[:, None] * dl
        nr = np.stack([np.zeros(M), pl[:, 1], pl[:, 2]], 1) / WHEEL_R
        n[better] = nr[better]
        t_in, t_out = np.where(better, lo, t_in), np.minimum(t_out, hi)
    return t_in, t_out, qrot(q, n)


def cast(qpos, block, px, py, camera=None):
    """shade the rays through image points (px, py) (flat arrays) -> dict of rgb [M, 3] float, depth, seg, shadow, checker
    and the entry parameter of every moving geom ("t": {seg id: t_in, inf where missed})"""
    c = cam_of(camera)
    fwd, up, right, pos, th = camera_frame(c)
    W, H = c["width"], c["height"]
    x = (2 * np.asarray(px, float) / W - 1) * th * W / H
    y = (1 - 2 * np.asarray(py, float) / H) * th
    d = fwd + x[:, None] * right + y[:, None] * up
    M = d.shape[0]
    o = np.broadcast_to(pos, (M, 3))
    L, qb, geoms = scene(qpos, block)
    best, seg, n = np.full(M, np.inf), np.zeros(M, int), np.zeros((M, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = (FLOOR_Z - L[2] - pos[2]) / d[:, 2]
    ok = (tf >= ZNEAR) & (tf <= ZFAR)
    best[ok], seg[ok] = tf[ok], SEG_FLOOR
    n[ok] = [0, 0, 1] if pos[2] >= FLOOR_Z - L[2] else [0, 0, -1]
    tmap = {}
    for gid, kind, cen, q, size in geoms:
        ti, to, ng = interval(kind, cen, q, size, o, d)
        hit = (ti <= to) & (ti >= ZNEAR) & (ti <= ZFAR)
        tmap[gid] = np.where(hit, ti, np.inf)
        nearer = hit & (ti < best)
        best[nearer], seg[nearer], n[nearer] = ti[nearer], gid, ng[nearer]
    vhat = d / np.linalg.norm(d, axis=1, keepdims=True)
    p = pos + best[:, None] * d
    albedo = np.zeros((M, 3))
    checker = np.full(M, -1)
    fl = seg == SEG_FLOOR
    par = (np.floor((L[0] + p[:, 0]) / CELL) + np.floor((L[1] + p[:, 1]) / CELL)).astype(np.int64) & 1
    checker[fl] = par[fl]
    albedo[fl] = np.where(par[fl, None] == 1, FLOOR_RGB[1], FLOOR_RGB[0])
    albedo[seg == SEG_TORSO] = TORSO_RGB
    albedo[seg == SEG_BLOCK] = BLOCK_RGB
    for w, gid in enumerate((SEG_WHEEL_L, SEG_WHEEL_R)):
        m = seg == gid
        ql = qrot(qinv(qb), p[m] - qrot(qb, WHEEL_POS[w]))
        phi = np.arctan2(ql[:, 2], ql[:, 1]) - WHEEL_AXIS_SIGN[w] * qpos[7 + w]
        sp = np.floor(phi / (2 * np.pi / SECTORS)).astype(np.int64) & 1
        checker[m] = sp
        albedo[m] = np.where(sp[:, None] == 1, WHEEL_RGB[1], WHEEL_RGB[0])
    ld = np.maximum(0, n @ TO_LIGHT)
    shadow = np.zeros(M, bool)
    lit = (seg >= SEG_FLOOR) & (ld > 0)
    for gid, kind, cen, q, size in geoms:
        m = lit & (seg != gid)
        if m.any():
            ti, to, _ = interval(kind, cen, q, size, p[m], TO_LIGHT)
            shadow[np.flatnonzero(m)[(ti <= to) & (to > 0)]] = True
    ld = np.where(shadow, 0, ld)
    hd = np.maximum(0, -np.einsum("ij,ij->i", n, vhat))
    rgb = albedo * (0.3 + 0.6 * hd + 0.7 * ld)[:, None]
    bg = seg == SEG_BG
    rgb[bg] = (0.4 * (vhat[bg, 2] + 1))[:, None]
    return dict(rgb=rgb, depth=best, seg=seg, shadow=shadow, checker=checker, t=tmap)


def render(qpos, block, camera=None, jitter=0.01):
    """one image -> rgb [H, W, 3] u8, depth [H, W] f32 (inf = background), seg [H, W] u8, ambiguous [H, W] bool"""
    c = cam_of(camera)
    W, H = c["width"], c["height"]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    px, py = jj.ravel(), ii.ravel()
    r = cast(qpos, block, px, py, c)
    amb = np.zeros(px.shape, bool)
    for dx, dy in ((jitter, 0), (-jitter, 0), (0, jitter), (0, -jitter)):
        s = cast(qpos, block, px + dx, py + dy, c)
        amb |= (s["seg"] != r["seg"]) | (s["shadow"] != r["shadow"]) | (s["checker"] != r["checker"])
    rgb = np.floor(np.clip(r["rgb"], 0, 1) * 255 + 0.5).astype(np.uint8)
    return (rgb.reshape(H, W, 3), r["depth"].astype(np.float32).reshape(H, W), r["seg"].astype(np.uint8).reshape(H, W),
            amb.reshape(H, W))


def _quat(axis, deg):
    a = np.radians(deg) / 2
    return np.concatenate([[np.cos(a)], np.sin(a) * np.asarray(axis, float) / np.linalg.norm(axis)])


def _qmul(p, q):
    w1, v1, w2, v2 = p[0], p[1:], q[0], q[1:]
    return np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + np.cross(v1, v2)])


def constructed_poses():
    """name -> Env03 qpos row (16): robot pos, quat, wheel angles, block pos, quat.  Env01 uses the first 9 columns."""
    up = np.array([1.0, 0, 0, 0])
    rest_z = FLOOR_Z  # wheel bottoms on the floor: body origin at floor height
    blk_far = np.concatenate([[0.6, -0.5, FLOOR_Z + BLOCK_HALF], up])
    p = {}
    p["upright"] = np.concatenate([[0.03, -0.02, rest_z], up, [1.3, -0.7], blk_far])
    t30 = _quat([1, 0, 0], 30)
    p["tilted30"] = np.concatenate([[0.0, 0.0, FLOOR_Z + WHEEL_R - WHEEL_POS[0][2] * np.cos(np.radians(30))], t30, [0.4, 2.2],
                                    blk_far])
    p["fallen"] = np.concatenate([[0.1, 0.05, FLOOR_Z + WHEEL_R], _quat([1, 0, 0], 90), [3.0, -3.0], blk_far])
    p["yawed"] = np.concatenate([[0.0, 0.0, rest_z], _quat([0, 0, 1], 100), [0.0, 0.3], blk_far])
    p["far60m"] = np.concatenate([[60.03, -42.71, rest_z], _qmul(_quat([0, 0, 1], -35), _quat([1, 0, 0], -12)), [345.6, -287.3],
                                  [60.5, -42.3, FLOOR_Z + BLOCK_HALF], _quat([0, 0, 1], 20)])
    p["block_flight"] = np.concatenate([[0.0, 0.0, rest_z], _quat([1, 0, 0], 8), [0.9, 0.9],
                                        [-0.25, -0.2, 0.15], _quat([1, 2, 3], 40)])
    # block against the outer face of the left wheel, resting on the floor
    p["block_wheel"] = np.concatenate([[0.0, 0.0, rest_z], up, [0.2, 0.1],
                                       [-WHEEL_POS[0][0] * -1 - WHEEL_HL - BLOCK_HALF, 0.0, FLOOR_Z + BLOCK_HALF], up])
    p["block_floor"] = np.concatenate([[0.0, 0.0, rest_z], _quat([0, 0, 1], -20), [0.0, 0.0],
                                       [0.25, -0.15, FLOOR_Z + BLOCK_HALF], _quat([0, 0, 1], 30)])
    return p
