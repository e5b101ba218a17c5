"""An independent float32 numpy restatement of the a-trous denoiser's contract (include/pt_hip.h,
"variance-guided a-trous denoiser"), written from the header text: vectorised over the pixels,
looping over the taps in the contract's order, every operation a float32 numpy operation of its
own. Also the variance of the mean from the moments, in float64, and the seeded synthetic inputs
the CPU and GPU tests share. None of the library's code is used here."""
import numpy as np

F32, F64 = np.float32, np.float64
H5 = [F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16)]
G3 = [F32(1 / 4), F32(1 / 2), F32(1 / 4)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    """Bits equal, or both NaN (NaN payloads differ between hosts and the GPU)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what=""):
    ok = same_bits(got, want)
    assert got.shape == want.shape and ok.all(), (
        f"{what}: {int((~ok).sum())} of {ok.size} values differ, first at {np.argwhere(~ok)[:3].tolist()}: "
        f"got {np.asarray(got)[~ok][:3]}, want {np.asarray(want)[~ok][:3]}")


def variance(S, Q, n):
    """m = S*S/n; d = (Q - m)/(n - 1); d = d > 0 ? d : 0; var = (float)(d/n); +inf for n < 2.
    n: an int, or an integer array with one count per pixel (S, Q: (..., 3))."""
    S, Q = np.asarray(S, dtype=F64), np.asarray(Q, dtype=F64)
    cnt = np.broadcast_to(np.asarray(n)[..., None] if np.ndim(n) else np.asarray(n), S.shape)
    dn = cnt.astype(F64)
    with np.errstate(all="ignore"):
        m = (S * S) / dn
        d = (Q - m) / (dn - F64(1))
        d = np.where(d > 0, d, F64(0))
        v = (d / dn).astype(F32)
    return np.where(cnt < 2, F32(np.inf), v).astype(F32)


def _shift(a, dy, dx):
    """(b, valid): b[y, x] = a[y + dy, x + dx] where that is inside the image."""
    H, W = a.shape[0], a.shape[1]
    b = np.zeros_like(a)
    valid = np.zeros((H, W), dtype=bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        valid[y0:y1, x0:x1] = True
    return b, valid


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def _lum(c):
    return ((F32(0.25) * c[..., 0]) + (F32(0.5) * c[..., 1])) + (F32(0.25) * c[..., 2])


def classes(tri, emission):
    return np.where(tri < 0, 0, np.where((emission != 0).any(axis=-1), 2, 1)).astype(np.int32)


def one_pass(c, v, nrm, X, tau, cls, s, sigma_l, npow, eps):
    H, W = cls.shape
    lum = _lum(c)
    den = None
    if v is not None:
        acc = np.zeros((H, W, 3), dtype=F32)
        wacc = np.zeros((H, W), dtype=F32)
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                vq, valid = _shift(v, j, k)
                g = G3[j + 1] * G3[k + 1]
                acc = np.where(valid[..., None], acc + g * vq, acc)
                wacc = np.where(valid, wacc + g, wacc)
        vt = acc / wacc[..., None]
        sig = ((F32(0.25) * np.sqrt(vt[..., 0])) + (F32(0.5) * np.sqrt(vt[..., 1]))) + (F32(0.25) * np.sqrt(vt[..., 2]))
        den = (F32(sigma_l) * sig) + F32(eps)
    A = np.zeros((H, W, 3), dtype=F32)
    B = np.zeros((H, W, 3), dtype=F32)
    Ws = np.zeros((H, W), dtype=F32)
    for j in range(-2, 3):
        for k in range(-2, 3):
            hh = H5[j + 2] * H5[k + 2]
            cq, ok = _shift(c, j * s, k * s)
            if j == 0 and k == 0:
                w = np.ones((H, W), dtype=F32)
            else:
                clq, _ = _shift(cls, j * s, k * s)
                ok = ok & (clq == cls)
                nq, _ = _shift(nrm, j * s, k * s)
                Xq, _ = _shift(X, j * s, k * s)
                dn = _dot(nrm, nq)
                dn = np.where(dn > 0, dn, F32(0))
                for _ in range(npow):
                    dn = dn * dn
                dl = np.abs(_dot(nrm, Xq - X))
                wz = np.where(dl < tau, (tau - dl) / tau, F32(0))
                wg = np.where(cls == 0, F32(1), dn * wz)
                if v is None:
                    wl = np.ones((H, W), dtype=F32)
                else:
                    lq, _ = _shift(lum, j * s, k * s)
                    xl = np.abs(lum - lq) / den
                    wl = F32(1) / (F32(1) + xl * xl)
                w = wg * wl
                ok = ok & (w > 0)
            kq = hh * w
            A = np.where(ok[..., None], A + kq[..., None] * cq, A)
            if v is not None:
                vq, _ = _shift(v, j * s, k * s)
                B = np.where(ok[..., None], B + (kq * kq)[..., None] * vq, B)
            Ws = np.where(ok, Ws + kq, Ws)
    c2 = A / Ws[..., None]
    v2 = B / (Ws * Ws)[..., None] if v is not None else None
    return c2.astype(F32), v2


def denoise(color, guides, var=None, passes=5, sigma_l=1.0, sigma_z=0.01, npow=7, eps=1e-6):
    """(out, var_out or None) by the contract's passes at strides 1, 2, 4, ..."""
    c = np.array(color, dtype=F32)
    H, W = c.shape[:2]
    v = None if var is None else np.array(var, dtype=F32)
    nrm = np.asarray(guides["normal"], dtype=F32).reshape(H, W, 3)
    X = np.asarray(guides["position"], dtype=F32).reshape(H, W, 3)
    t = np.asarray(guides["t"], dtype=F32).reshape(H, W)
    cls = classes(np.asarray(guides["tri"]).reshape(H, W), np.asarray(guides["emission"], dtype=F32).reshape(H, W, 3))
    with np.errstate(all="ignore"):
        tau = F32(sigma_z) * t
        for i in range(passes):
            c, v = one_pass(c, v, nrm, X, tau, cls, 1 << i, sigma_l, npow, eps)
    return c, v


def tri_normal(verts, tri, d):
    """Triangle::normal (triangle.h:45-49) in float32: edge1 x edge2, / length, n . d < 0 ? n : -n."""
    v = verts[tri].astype(F32)
    e1, e2 = v[..., 3:6] - v[..., 0:3], v[..., 6:9] - v[..., 0:3]
    x1, y1, z1 = e1[..., 0], e1[..., 1], e1[..., 2]
    x2, y2, z2 = e2[..., 0], e2[..., 1], e2[..., 2]
    cx, cy, cz = y1 * z2 - z1 * y2, z1 * x2 - x1 * z2, x1 * y2 - y1 * x2
    ln = np.sqrt(cx * cx + cy * cy + cz * cz)
    n = np.stack([cx / ln, cy / ln, cz / ln], axis=-1)
    dot = n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]
    return np.where((dot < 0)[..., None], n, -n).astype(F32)


NORMALS = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0.8, 0], [0, 0, -1]], dtype=F32)


def synthetic(W, H, seed=0, nasty=True):
    """Seeded inputs (color, var, guides) of a W x H image with all three classes, four surface
    orientations in blocks, hit points near a plane with a jitter of the order of tau, and, with
    `nasty`, NaN, +-inf, negative and NaN and +inf variance, t = 0, denormals and values near 2^100
    at seeded pixels (where the image has room for them)."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    color = rng.uniform(0, 2, (H, W, 3)).astype(F32)
    color += (0.5 * ((xx // 5 + yy // 4) % 3))[..., None].astype(F32)
    var = (rng.uniform(0.001, 0.3, (H, W, 3)) ** 2).astype(F32)
    region = (xx // 6 + 2 * (yy // 5)) % 4
    normal = NORMALS[region]
    pos = np.stack([0.1 * xx, 0.1 * yy, 5 + 0.02 * rng.standard_normal((H, W))], axis=-1).astype(F32)
    t = rng.uniform(3, 8, (H, W)).astype(F32)
    tri = rng.integers(0, 12, (H, W)).astype(np.int32)
    emission = np.zeros((H, W, 3), dtype=F32)
    kind = (xx // 7 + yy // 6) % 5  # 0: miss, 1: emitter, else a plain hit
    if W * H > 2:
        flat = kind.reshape(-1)
        flat[0], flat[1], flat[2] = 0, 1, 2  # all three classes present
    miss, emit = kind == 0, kind == 1
    tri[miss] = -1
    t[miss] = F32(1e30)
    normal = np.where(miss[..., None], F32(0), normal).astype(F32)
    emission[emit] = rng.choice(np.array([[1, 1, 1], [0, 0.5, 0], [0, 0, 2]], dtype=F32), int(emit.sum()))
    if nasty and W * H >= 20:
        p = rng.permutation(W * H)[:14]
        cf, vf, tf = color.reshape(-1, 3), var.reshape(-1, 3), t.reshape(-1)
        cf[p[0], 1] = np.nan
        cf[p[1], 0] = np.inf
        cf[p[2], 2] = -np.inf
        vf[p[3], 1] = -0.01
        vf[p[4], 0] = np.nan
        vf[p[5]] = np.inf
        tf[p[6]] = 0
        cf[p[7]] = F32(1e-42)
        vf[p[8]] = F32(1e-44)
        cf[p[9]] = F32(2.0 ** 100)
        vf[p[10]] = F32(2.0 ** 100)
        cf[p[11], 0] = F32(-(2.0 ** 100))
        pos.reshape(-1, 3)[p[12]] = F32(2.0 ** 100)
        normal.reshape(-1, 3)[p[13]] = np.nan
    guides = {"normal": np.ascontiguousarray(normal), "t": t, "tri": tri, "emission": emission,
              "position": np.ascontiguousarray(pos)}
    return color, var, guides
