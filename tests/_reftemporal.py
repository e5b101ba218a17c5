"""An independent float32 numpy restatement of the temporal reprojection's contract
(include/pt_hip.h, "temporal reprojection"), written from the header text: vectorised over the
pixels, looping over the four taps in the contract's order, every operation a float32 numpy
operation of its own. Also the seeded synthetic frames the CPU and GPU tests share: a few tilted
planes seen by two cameras, with a random previous history and planted cases. None of the
library's code is used here."""
from types import SimpleNamespace

import numpy as np

from _refdenoise import F32, assert_same, bits, classes, same_bits  # noqa: F401

I32 = np.int32
NAMES = ("color", "m2", "var", "hist", "normal", "position", "cls")
SAMPLE, TEMPORAL = 1, 2
MOVES = ("none", "subpixel", "pixels", "far", "turned")
INF = F32(np.inf)


def cam_fields(c):
    """The fields proj() reads, from anything with pt_camera's members (a ctypes pt_camera, or the
    generator's own namespace)."""
    return SimpleNamespace(pos=np.array(list(c.pos), dtype=F32), v_res=np.array(list(c.v_res), dtype=F32),
                           cell=F32(c.cell_size), dist=F32(c.distance),
                           T=np.array(list(c.transform), dtype=F32).reshape(3, 3))


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def proj(cam, X):
    """(fx, fy, valid) of the contract's proj(cam, X)."""
    d = X - cam.pos
    cx, cy, cz = _dot(d, cam.T[0]), _dot(d, cam.T[1]), _dot(d, cam.T[2])
    valid = cz < 0
    k = (F32(0) - cam.dist) / cz
    fx = ((cx * k) + (F32(0.5) * cam.v_res[0])) / cam.cell
    fy = ((cy * k) + (F32(0.5) * cam.v_res[1])) / cam.cell
    return fx, fy, valid


def accumulate(color, guides, cam_cur, cam_prev=None, prev=None, var=None, max_history=32, sigma_z=0.01,
               normal_min=0.9, mode=0):
    """(next: dict of the seven planes, reused) by the contract's steps 1-7. prev: a dict of the
    seven planes or None; cameras: anything cam_fields() reads."""
    c = np.asarray(color, dtype=F32)
    H, W = c.shape[:2]
    sample = (var is not None) if mode == 0 else mode == SAMPLE
    v = np.asarray(var, dtype=F32) if sample else None
    n = np.asarray(guides["normal"], dtype=F32).reshape(H, W, 3)
    X = np.asarray(guides["position"], dtype=F32).reshape(H, W, 3)
    t = np.asarray(guides["t"], dtype=F32).reshape(H, W)
    cls = classes(np.asarray(guides["tri"]).reshape(H, W), np.asarray(guides["emission"], dtype=F32).reshape(H, W, 3))
    yy, xx = np.mgrid[0:H, 0:W]
    A = np.zeros((H, W, 3), dtype=F32)
    M = np.zeros((H, W, 3), dtype=F32)
    V = np.zeros((H, W, 3), dtype=F32)
    Wsum = np.zeros((H, W), dtype=F32)
    Nmin = np.full((H, W), np.iinfo(I32).max, dtype=I32)
    with np.errstate(all="ignore"):
        if prev is not None:
            cur, old = cam_fields(cam_cur), cam_fields(cam_prev)
            fxc, fyc, okc = proj(cur, X)
            fxp, fyp, okp = proj(old, X)
            gx = xx.astype(F32) + (fxp - fxc)
            gy = yy.astype(F32) + (fyp - fyc)
            cand = (cls != 0) & okc & okp & (gx > F32(-1)) & (gx < F32(W)) & (gy > F32(-1)) & (gy < F32(H))
            gx, gy = np.where(cand, gx, F32(0)), np.where(cand, gy, F32(0))
            x0, y0 = np.floor(gx).astype(I32), np.floor(gy).astype(I32)
            ax, ay = gx - x0.astype(F32), gy - y0.astype(F32)
            wx, wy = [F32(1) - ax, ax], [F32(1) - ay, ay]
            tau = F32(sigma_z) * t
            P = {k: np.asarray(prev[k]) for k in NAMES if prev.get(k) is not None}
            for j in (0, 1):
                for k in (0, 1):
                    qx, qy = x0 + k, y0 + j
                    ok = cand & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    bw = wx[k] * wy[j]
                    hq = P["hist"].reshape(H, W)[qy, qx]
                    cq = P["color"].reshape(H, W, 3)[qy, qx].astype(F32)
                    nq = P["normal"].reshape(H, W, 3)[qy, qx].astype(F32)
                    Xq = P["position"].reshape(H, W, 3)[qy, qx].astype(F32)
                    ok &= bw > 0
                    ok &= hq >= 1
                    ok &= P["cls"].reshape(H, W)[qy, qx] == cls
                    ok &= _dot(n, nq) > F32(normal_min)
                    ok &= np.abs(_dot(n, Xq - X)) < tau
                    ok &= (np.abs(cq) < INF).all(axis=-1)
                    Wsum = np.where(ok, Wsum + bw, Wsum)
                    A = np.where(ok[..., None], A + bw[..., None] * cq, A)
                    M = np.where(ok[..., None], M + bw[..., None] * P["m2"].reshape(H, W, 3)[qy, qx].astype(F32), M)
                    if sample:
                        V = np.where(ok[..., None], V + bw[..., None] * P["var"].reshape(H, W, 3)[qy, qx].astype(F32), V)
                    Nmin = np.where(ok, np.minimum(Nmin, hq), Nmin)
        reuse = Wsum > 0
        N = np.where(reuse, np.minimum(Nmin, I32(max_history - 1)) + I32(1), I32(1)).astype(I32)
        alpha = (F32(1) / N.astype(F32))[..., None]
        b = F32(1) - alpha
        Ws = Wsum[..., None]
        c_acc = (b * (A / Ws)) + (alpha * c)
        m_acc = (b * (M / Ws)) + (alpha * (c * c))
        if sample:
            v_acc = ((b * b) * (V / Ws)) + ((alpha * alpha) * v)
            v_new = v
        else:
            d = m_acc - (c_acc * c_acc)
            d = np.where(d > 0, d, F32(0))
            v_acc = d * alpha
            v_new = np.full((H, W, 3), INF, dtype=F32)
        r3 = reuse[..., None]
        nxt = {"color": np.where(r3, c_acc, c).astype(F32), "m2": np.where(r3, m_acc, c * c).astype(F32),
               "var": np.where(r3, v_acc, v_new).astype(F32), "hist": N, "normal": n.copy(), "position": X.copy(),
               "cls": cls.copy()}
    return nxt, int(reuse.sum())


# ---------------------------------------------------------------- the synthetic frames
FOV = 1.0  # radians


def _camera(pos, W, H, back=False):
    """pt_camera's members for a camera at `pos` looking down -z (or, `back`, down +z), up = +y:
    the arithmetic of camera.h:50-60 in float32. Rows: right, up, -forward."""
    vx = F32(2 * np.tan(FOV / 2))
    s = F32(-1) if back else F32(1)
    return SimpleNamespace(pos=[F32(p) for p in pos], res=[W, H], v_res=[vx, F32(vx * F32(H) / F32(W))],
                           cell_size=F32(vx / F32(W)), distance=F32(1),
                           transform=[s, 0, 0, 0, 1, 0, 0, 0, s], back=back)


def camera_spec(cam):
    """(pos, forward, up, res, fov, distance): what a library camera is made from."""
    return (tuple(float(p) for p in cam.pos), (0.0, 0.0, 1.0 if cam.back else -1.0), (0.0, 1.0, 0.0), tuple(cam.res), FOV, 1.0)


PLANES = {  # kind -> (unit normal towards the camera, a point): flat, tilted in x, tilted in y
    1: ((0.0, 0.0, 1.0), (0.0, 0.0, -6.0)), 2: ((0.0, 0.0, 1.0), (0.0, 0.0, -6.0)),
    3: ((-0.6, 0.0, 1.0), (0.0, 0.0, -6.0)), 4: ((0.0, 0.7, 1.0), (0.0, 0.0, -6.0)),
}


def _view(cam, W, H, rng):
    """The world seen from `cam` through one jittered ray per pixel: (normal, t, tri, emission,
    position). The world is cut into square blocks on the plane z = -6; a block is a miss, an
    emitter on the flat plane, or one of three planes."""
    f = cam_fields(cam)
    yy, xx = np.mgrid[0:H, 0:W]
    jx, jy = rng.uniform(0, 1, (H, W)).astype(F32), rng.uniform(0, 1, (H, W)).astype(F32)
    if W * H < 20:  # a tiny image's pixels span whole blocks: rays through the centres, so that two views can agree
        jx, jy = np.full((H, W), 0.5, dtype=F32), np.full((H, W), 0.5, dtype=F32)
    dc = np.stack([(xx + jx) * f.cell - f.v_res[0] / F32(2), (yy + jy) * f.cell - f.v_res[1] / F32(2),
                   np.full((H, W), -f.dist, dtype=F32)], axis=-1).astype(F32)
    d = np.stack([_dot(dc, f.T[:, k]) for k in range(3)], axis=-1).astype(F32)
    d = (d / np.sqrt(_dot(d, d))[..., None]).astype(F32)
    o = f.pos
    t0 = (F32(-6) - o[2]) / d[..., 2]
    base = o + d * t0[..., None]
    block = F32(6 * 6) * F32(2 * np.tan(FOV / 2) / 37)  # about 6 pixels of a 37-pixel-wide image at z = -6
    kind = ((np.floor(base[..., 0] / block) + 2 * np.floor(base[..., 1] / block) + 2) % 5).astype(I32)  # the block at the origin: flat
    kind = np.where(t0 > 0, kind, 0)
    normal = np.zeros((H, W, 3), dtype=F32)
    t = np.full((H, W), 1e30, dtype=F32)
    for k, (nk, pk) in PLANES.items():
        nk = np.array(nk, dtype=F32)
        nk = (nk / np.sqrt(_dot(nk, nk))).astype(F32)
        tk = (_dot(nk, np.array(pk, dtype=F32) - o) / _dot(d, nk)).astype(F32)
        m = kind == k
        normal[m] = nk
        t[m] = tk[m]
    miss = kind == 0
    tri = np.where(miss, -1, kind).astype(I32)
    emission = np.zeros((H, W, 3), dtype=F32)
    emission[kind == 1] = F32(2)
    m = (d * t[..., None]).astype(F32)
    return {"normal": normal, "t": t, "tri": tri, "emission": emission, "position": (o + m).astype(F32)}


def _rotated(n, cos):
    """Unit vectors at angle acos(cos) from the unit vectors n."""
    u = np.cross(n, np.array([0.3, 0.5, 0.2], dtype=F32))
    u = u / np.maximum(np.sqrt((u * u).sum(axis=-1, keepdims=True)), 1e-20)
    return (cos * n + np.sqrt(1 - cos * cos) * u).astype(F32)


def synthetic(W, H, seed=0, move="pixels"):
    """Seeded inputs of one call: a namespace with cam_cur, cam_prev (pt_camera's members; make
    library cameras from camera_spec()), color, var, guides (the current frame) and prev (a dict
    of the seven planes). `move` is the previous camera's offset: "none" (the same camera),
    "subpixel", "pixels" (3.4 and 1.7 pixels at the scene's depth), "far" (most of the frame
    leaves the image) and "turned" (the previous camera looks the other way: cz >= 0).

    The previous history's colour, m2, var and hist are random; planted in it (where the image has
    room): NaN and +inf colours, hist at and above the default max_history, hist == 0 holes (a
    block and single pixels), a block whose class differs from what the current frame sees there,
    and normals just either side of the default normal_min."""
    rng = np.random.default_rng(7000 + 31 * seed + MOVES.index(move))
    px = F32(6) * F32(2 * np.tan(FOV / 2)) / F32(W)  # a pixel's width at z = -6
    off = {"none": (0, 0), "subpixel": (0.3, -0.2), "pixels": (3.4, 1.7), "far": (0.8 * W, 0.0), "turned": (0, 0)}[move]
    cam_cur = _camera((0.0, 0.0, 0.0), W, H)
    cam_prev = _camera((off[0] * px, off[1] * px, 0.0), W, H, back=move == "turned") if move != "none" else cam_cur
    guides = _view(cam_cur, W, H, rng)
    # "turned": the history is the current view itself, so only cz >= 0 keeps it from being reused
    old = _view(cam_cur if move == "turned" else cam_prev, W, H, rng)
    color = rng.uniform(0, 2, (H, W, 3)).astype(F32)
    var = (rng.uniform(0.001, 0.3, (H, W, 3)) ** 2).astype(F32)
    prev = {"color": rng.uniform(0, 2, (H, W, 3)).astype(F32), "m2": rng.uniform(0, 4, (H, W, 3)).astype(F32),
            "var": (rng.uniform(0.001, 0.2, (H, W, 3)) ** 2).astype(F32),
            "hist": rng.integers(1, 31, (H, W)).astype(I32), "normal": old["normal"].copy(),
            "position": old["position"].copy(), "cls": classes(old["tri"], old["emission"])}
    if W * H >= 20:
        yy, xx = np.mgrid[0:H, 0:W]
        hole = (yy >= H // 4) & (yy < H // 2) & (xx < W // 2)
        prev["hist"][hole] = 0
        swap = (yy >= (2 * H) // 3) & (xx >= (2 * W) // 3)  # a class change across the block's edges
        prev["cls"][swap] = np.where(prev["cls"][swap] == 1, 2, 1)
        tilt = (yy < H // 5) & (xx >= W // 2)  # normals just either side of normal_min
        cos = np.where((xx + yy) % 2 == 0, 0.9 + 2e-3, 0.9 - 2e-3)[..., None]
        prev["normal"][tilt] = _rotated(prev["normal"], cos)[tilt]
        # single pixels, on hits outside the blocks where there are enough of them
        free = np.flatnonzero(((prev["cls"] != 0) & ~hole & ~swap & ~tilt).reshape(-1))
        p = rng.permutation(free if free.size >= 12 else W * H)[:12]
        cf, hf = prev["color"].reshape(-1, 3), prev["hist"].reshape(-1)
        cf[p[0], 1] = np.nan
        cf[p[1], 0] = np.inf
        cf[p[2]] = np.nan
        cf[p[3], 2] = -np.inf
        hf[p[4]], hf[p[5]], hf[p[6]], hf[p[7]] = 31, 32, 33, 60000
        hf[p[8]], hf[p[9]] = 0, -3
        color.reshape(-1, 3)[p[10], 0] = np.nan  # a NaN of the current frame stays in its pixel
        prev["m2"].reshape(-1, 3)[p[11]] = F32(1e-42)
    return SimpleNamespace(W=W, H=H, cam_cur=cam_cur, cam_prev=cam_prev, color=color, var=var, guides=guides, prev=prev)
