"""The vertex-colour bake contract (include/forge_hip.h section g2) restated in numpy, and the scenes the bake tests run on.

reference_bake computes in float64 from the float32 inputs the kernel gets; dtype=np.float32 reruns the same formulas in fp32 (products combined in
the contract's fixed order): the difference of the two is the precision yardstick of tests/test_gpu_bake.py. The vertices come from
mesh_cases.reference_mesh, rounded to float32, so no GPU is needed here. Used by tests/test_bake_cpu.py and tests/test_gpu_bake.py."""
import math

import numpy as np

import mesh_cases as mc

GROUP = 8          # the contract's combination order: partial products over s = j (mod 8), then pairs j ^ 1, j ^ 2, j ^ 4


# ----------------------------------------------------------------------------------------------------------------------------- cameras
def look_at(center, target=(0.0, 0.0, 0.0), down=(0.0, 1.0, 0.0)):
    """OpenCV world->camera (R [3,3], T [3]) of a camera at `center` looking at `target` (z forward, x right, y down)."""
    c = np.asarray(center, np.float64)
    z = np.asarray(target, np.float64) - c
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(down, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def orbit(V, dist=1.5, elev_deg=0.0, phase_deg=0.0):
    """V camera centres on a circle of radius dist around the origin: azimuth about the y axis, elevation elev_deg (a number or V numbers)."""
    elev = np.broadcast_to(np.deg2rad(np.asarray(elev_deg, np.float64)), (V,))
    azim = np.deg2rad(phase_deg) + 2.0 * math.pi * np.arange(V) / V
    return [(dist * math.cos(e) * math.sin(a), dist * math.sin(e), dist * math.cos(e) * math.cos(a)) for a, e in zip(azim, elev)]


def pack(centers, Hi, Wi, focal=1.38888):
    """cam [V,16] float32: R, T, fx = focal Wi, fy = focal Hi, cx = Wi / 2, cy = Hi / 2 (pixels of Hi x Wi images)."""
    rows = []
    for c in centers:
        R, T = look_at(c)
        rows.append(np.concatenate([R.reshape(9), T, [focal * Wi, focal * Hi, 0.5 * Wi, 0.5 * Hi]]))
    return np.asarray(rows, np.float32)


def half_extents(shape, volume_size=1.0):
    D, H, W = shape
    return tuple(0.5 * (N - 1) * volume_size / N for N in (W, H, D))


def defaults(shape, volume_size=1.0):
    """(step, S, offset) as geometry.bake_vertex_colors chooses them."""
    step = volume_size / max(shape)
    return step, int(math.ceil(1.8 * volume_size / step)), step


# ----------------------------------------------------------------------------------------------------------------------- the restatement
def trilinear(dens, px, py, pz):
    """The zero-padded align_corners=True sample of dens [D,H,W] at index positions (px, py, pz) <-> (W, H, D), in dens.dtype."""
    dt = dens.dtype.type
    D, H, W = dens.shape
    px, py, pz = np.clip(px, dt(-2), dt(W + 1)), np.clip(py, dt(-2), dt(H + 1)), np.clip(pz, dt(-2), dt(D + 1))
    fx, fy, fz = np.floor(px), np.floor(py), np.floor(pz)
    x0, y0, z0 = fx.astype(np.int64), fy.astype(np.int64), fz.astype(np.int64)
    wx, wy, wz = ((fx + dt(1)) - px, px - fx), ((fy + dt(1)) - py, py - fy), ((fz + dt(1)) - pz, pz - fz)
    out = np.zeros(px.shape, dens.dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = x0 + dx, y0 + dy, z0 + dz
                ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & (zi >= 0) & (zi < D)
                val = dens[np.clip(zi, 0, D - 1), np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
                out = out + np.where(ok, wx[dx] * wy[dy] * wz[dz] * val, dt(0))
    return out


class Baked:
    def __init__(self, colors, weight, best, per_view, margin):
        self.colors, self.weight, self.best = colors, weight, best
        self.per_view = per_view          # [V, rows] the w_v (0 for views of other volumes)
        self.margin = margin              # min over rows and the volume's views of the distance (pixels / depth units) to the in-view test's boundary

    def top_two_gap(self):
        w = np.sort(self.per_view.astype(np.float64), axis=0)
        return w[-1] - (w[-2] if w.shape[0] > 1 else 0.0)


def reference_bake(vertices, normals, density, half, images, cam, view2vol, vol=0, view_weight=None, view_gain=None, *, S, step, offset, cos_power=2,
                   z_near=1e-3, w_min=1e-3, mode=0, fill=0.5, dtype=np.float64):
    """One volume's rows: vertices / normals [rows,3], density [D,H,W], images [V,C,Hi,Wi], cam [V,16], view2vol [V] (all views of the call; the
    volume `vol` looks at its own) -> Baked. The inputs are the float32 arrays the kernel gets."""
    dt = dtype
    one, zero = dt(1), dt(0)
    P, Nh = np.asarray(vertices, np.float32).astype(dt), np.asarray(normals, np.float32).astype(dt)
    dens = np.asarray(density, np.float32).astype(dt)
    D, H, W = dens.shape
    img = np.asarray(images, np.float32).astype(dt)
    V, C, Hi, Wi = img.shape
    cams = np.asarray(cam, np.float32).astype(dt)
    hx, hy, hz = (dt(np.float32(h)) for h in half)
    step, offset, z_near, w_min, fill = (dt(np.float32(v)) for v in (step, offset, z_near, w_min, fill))
    rows = P.shape[0]
    flat = (Nh == 0).all(axis=1)
    P0 = np.where(flat[:, None], P, P + offset * Nh)
    weight, acc = np.zeros(rows, dt), np.zeros((rows, C), dt)
    wbest, cbest, best = np.zeros(rows, dt), np.zeros((rows, C), dt), np.full(rows, -1, np.int32)
    per_view = np.zeros((V, rows), dt)
    margin = np.inf
    with np.errstate(all="ignore"):
        for v in range(V):
            if int(view2vol[v]) != vol:
                continue
            R, T, (fx, fy, cx, cy) = cams[v, :9].reshape(3, 3), cams[v, 9:12], cams[v, 12:16]
            xc = R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + T[0]
            yc = R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + T[1]
            zc = R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + T[2]
            x, y = (fx * xc) / zc + cx - dt(0.5), (fy * yc) / zc + cy - dt(0.5)
            front = zc >= z_near
            inside = np.minimum(np.minimum(x, dt(Wi - 1) - x), np.minimum(y, dt(Hi - 1) - y))
            seen = front & (inside >= zero)
            if rows:
                margin = min(margin, float(np.abs(zc - z_near).min()), float(np.abs(inside[front]).min()) if front.any() else np.inf)
            xs, ys = np.where(seen, x, zero), np.where(seen, y, zero)
            fx0, fy0 = np.floor(xs), np.floor(ys)
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, Wi - 1), np.minimum(y0 + 1, Hi - 1)
            ax, ay = xs - fx0, ys - fy0
            w00, w01, w10, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay

            def tap(plane):
                return w00 * plane[y0, x0] + w01 * plane[y0, x1] + w10 * plane[y1, x0] + w11 * plane[y1, x1]
            m = np.ones(rows, dt) if view_weight is None else tap(np.asarray(view_weight[v], np.float32).astype(dt))
            c = np.stack([tap(img[v, k]) for k in range(C)], axis=1)
            cen = -(R.T @ T)
            d = cen[None, :] - P
            dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            u = d / dist[:, None]
            cosine = np.maximum(Nh[:, 0] * u[:, 0] + Nh[:, 1] * u[:, 1] + Nh[:, 2] * u[:, 2], zero)
            facing = cosine.copy()
            for _ in range(1, cos_power):
                facing = facing * cosine
            facing = np.where(flat, one, facing)
            part = [np.ones(rows, dt) for _ in range(GROUP)]
            for s in range(S):
                t = dt(s + 0.5) * step
                pos = P0 + t * u
                px = (((pos[:, 0] / hx) + one) / dt(2)) * dt(W - 1)
                py = (((pos[:, 1] / hy) + one) / dt(2)) * dt(H - 1)
                pz = (((pos[:, 2] / hz) + one) / dt(2)) * dt(D - 1)
                a = np.where(t < dist, np.clip(trilinear(dens, px, py, pz), zero, one), zero)
                part[s % GROUP] = part[s % GROUP] * (one - a)
            for k in (1, 2, 4):
                part = [part[j] * part[j ^ k] for j in range(GROUP)]
            gain = one if view_gain is None else dt(np.float32(view_gain[v]))
            w = np.where(seen, gain * m * part[0] * facing, zero)
            per_view[v] = w
            weight = weight + w
            acc = acc + w[:, None] * c
            better = w > wbest
            wbest, best = np.where(better, w, wbest), np.where(better, np.int32(v), best)
            cbest = np.where(better[:, None], c, cbest)
        filled = (best < 0) | ~(weight >= w_min)
        colors = np.where(filled[:, None], fill, acc / weight[:, None] if mode == 0 else cbest)
    return Baked(colors, weight, best, per_view, margin)


# -------------------------------------------------------------------------------------------------------------------------------- scenes
_MESH = {}


def ref_mesh32(key, build, level=0.5, volume_size=1.0):
    """(density float32, vertices float32, normals float32, faces int32) of mesh_cases.reference_mesh on build(); computed once per process."""
    if key not in _MESH:
        dens = build()
        m = mc.reference_mesh(dens, level, volume_size)
        _MESH[key] = (dens, m.vertices.astype(np.float32), m.normals.astype(np.float32), m.faces)
    return _MESH[key]


def random_images(V, C, Hi, Wi, seed):
    return np.random.default_rng(seed).random((V, C, Hi, Wi), dtype=np.float32)


class Scene:
    """What one bake call gets, as numpy: volumes (list of (density, vertices, normals, faces)), images, cam, view2vol, optional maps and gains, knobs."""

    def __init__(self, volumes, images, cam, view2vol, volume_size=1.0, view_weight=None, view_gain=None, **knobs):
        self.volumes, self.images, self.cam, self.view2vol = volumes, images, cam, np.asarray(view2vol, np.int32)
        self.volume_size, self.view_weight, self.view_gain = volume_size, view_weight, view_gain
        shape = volumes[0][0].shape
        step, S, offset = defaults(shape, volume_size)
        self.knobs = dict(S=S, step=step, offset=offset)
        self.knobs.update(knobs)
        self.half = half_extents(shape, volume_size)

    def reference(self, dtype=np.float64, **over):
        kw = dict(self.knobs)
        kw.update(over)
        return [reference_bake(v, nr, d, self.half, self.images, self.cam, self.view2vol, k, self.view_weight, self.view_gain, dtype=dtype, **kw)
                for k, (d, v, nr, _) in enumerate(self.volumes)]


def scene(name):
    if name == "blob8_one_view":
        return Scene([ref_mesh32("blob8", lambda: mc.blob(8))], random_images(1, 3, 16, 16, 1), pack(orbit(1, phase_deg=20.0, elev_deg=15.0), 16, 16), [0], S=13)
    if name == "ellipsoid16_orbit6":
        return Scene([ref_mesh32("ellipsoid16", lambda: mc.ellipsoid(16))], random_images(6, 3, 32, 32, 2), pack(orbit(6, phase_deg=10.0), 32, 32), [0] * 6,
                     cos_power=2)
    if name == "blob16_off_centre_maps":
        V = 7
        rng = np.random.default_rng(3)
        return Scene([ref_mesh32("blob16_off", lambda: mc.blob(16, (0.05, -0.03, 0.02)))], random_images(V, 4, 16, 24, 4),
                     pack(orbit(V, phase_deg=5.0, elev_deg=np.linspace(-30.0, 30.0, V)), 16, 24), [0] * V,
                     view_weight=(0.5 + 0.5 * rng.random((V, 16, 24))).astype(np.float32), view_gain=(0.5 + rng.random(V)).astype(np.float32), cos_power=3)
    if name == "noncubic_6x5x7":
        return Scene([ref_mesh32("noncubic", mc.noncubic, mc.QUANT_LEVEL, 1.5)], random_images(3, 3, 20, 20, 5),
                     pack(orbit(3, dist=3.0, phase_deg=25.0, elev_deg=(10.0, -20.0, 35.0)), 20, 20), [0] * 3, volume_size=1.5)
    if name == "two_blobs8_interleaved":
        vols = [ref_mesh32("blob8_a", lambda: mc.blob(8, (0.06, -0.04, 0.02))), ref_mesh32("blob8_b", lambda: mc.blob(8, (-0.05, 0.03, -0.07)))]
        return Scene(vols, random_images(6, 3, 16, 16, 6), pack(orbit(6, phase_deg=15.0, elev_deg=(0.0, 20.0, -20.0, 10.0, -10.0, 0.0)), 16, 16),
                     [0, 1, 0, 7, 1, 0])                       # view 3 names a volume that does not exist: ignored
    raise KeyError(name)


def hand_made_rows():
    """Rows a mesh never produces, on blob(8) with two cameras: (density, vertices, normals, cam, images). Rows 0..5: a normal row, the same point with
    a zero normal (facing 1, no offset), a vertex behind the cameras, one projecting outside the images, an oblique row, a zero normal on the far
    side. Then 58 ordinary rows in the ball of radius 0.4 with random unit normals, so that the case's fp32 yardstick is not six rows' luck."""
    p = np.array([[0.0, 0.0, -0.35], [0.0, 0.0, -0.35], [0.0, 0.0, -2.0], [1.2, 0.0, 0.0], [0.1, -0.2, -0.3], [0.0, 0.0, 0.35]], np.float32)
    nh = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, -0.6, -0.8], [0.0, 0.0, 0.0]], np.float32)
    rng = np.random.default_rng(17)
    q = rng.standard_normal((58, 3))
    p = np.concatenate([p, (0.4 * rng.random((58, 1)) ** (1 / 3) * q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)])
    q = rng.standard_normal((58, 3))
    nh = np.concatenate([nh, (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)])
    return mc.blob(8), p, nh, pack([(0.0, 0.0, -1.5), (0.3, 0.2, -1.4)], 16, 16), random_images(2, 2, 16, 16, 9)


SCENES = ("blob8_one_view", "ellipsoid16_orbit6", "blob16_off_centre_maps", "noncubic_6x5x7", "two_blobs8_interleaved")
