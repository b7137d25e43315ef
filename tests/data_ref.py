"""float64 numpy evaluation of the formulas of include/lgm_data.h: the truth of tests/test_data_gpu.py and the check
tests/golden/make_data_golden.py runs on the recorded reference outputs. Written from the header, sharing no code with
lgm_amd/data.py."""
import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def affine(m):
    """[..., 4, 4] -> float64 with the last row taken as (0, 0, 0, 1)."""
    m = np.array(m, np.float64)
    m[..., 3, :] = (0, 0, 0, 1)
    return m


def rodrigues(r):
    th = float(np.linalg.norm(r))
    a = 1.0 if th == 0 else math.sin(th) / th
    hb = 1.0 if th == 0 else math.sin(th / 2) / (th / 2)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], np.float64)
    return np.eye(3) + a * K + 0.5 * hb * hb * (K @ K)


def jitter64(P, u, strength):
    """One pose [4, 4] (as float32 holds it) and u = (u0, u1) -> the jittered pose, float64."""
    P = affine(P)
    rot = rodrigues(P[:3, 1] * strength * math.pi * float(u[0])) @ rodrigues(P[:3, 0] * strength * math.pi / 2 * float(u[1]))
    out = P.copy()
    out[:3, :3] = rot @ P[:3, :3]
    out[:3, 3] = rot @ P[:3, 3]
    return out


def proj32(fovy, znear, zfar):
    p = np.zeros((4, 4), np.float32)
    p[0, 0] = p[1, 1] = 1 / math.tan(0.5 * math.radians(fovy))
    p[2, 2] = (zfar + znear) / (zfar - znear)
    p[3, 2] = -(zfar * znear) / (zfar - znear)
    p[2, 3] = 1
    return p.astype(np.float64)


def cameras64(c2w, Vi, jitter, strength, radius, fovy, znear, zfar):
    """c2w [B, V, 4, 4] float32 -> dict of float64 arrays: P (the normalised pose before its float32 rounding), pose_in,
    c2w_colmap, cam_view, cam_view_proj, cam_pos."""
    c2w = affine(c2w)
    B, V = c2w.shape[:2]
    T = np.eye(4)
    T[2, 3] = radius
    P = np.stack([np.stack([T @ np.linalg.inv(c2w[b, 0]) @ c2w[b, v] for v in range(V)]) for b in range(B)])
    P32 = P.astype(np.float32).astype(np.float64)
    pose_in = P32[:, :Vi].copy()
    if jitter is not None:
        for b in range(B):
            for v in range(Vi):
                pose_in[b, v] = jitter64(P32[b, v], jitter[b, v], strength)
    Pf = P32.copy()
    Pf[..., :3, 1:3] *= -1
    cam_view = np.swapaxes(np.linalg.inv(Pf), -1, -2)
    return {"P": P, "pose_in": pose_in, "c2w_colmap": Pf[:, :Vi], "cam_view": cam_view,
            "cam_view_proj": cam_view @ proj32(fovy, znear, zfar), "cam_pos": -Pf[..., :3, 3]}


def taps(S, R):
    d = np.arange(R, dtype=np.float64)
    s = np.maximum((d + 0.5) * S / R - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), S - 1)
    return i0, np.minimum(i0 + 1, S - 1), s - i0


def resize64(f, R):
    """f [..., Hs, Ws] float64 -> [..., R, R], bilinear, align_corners = False."""
    y0, y1, ly = taps(f.shape[-2], R)
    x0, x1, lx = taps(f.shape[-1], R)
    top = (1 - lx) * f[..., y0, :][..., x0] + lx * f[..., y0, :][..., x1]
    bot = (1 - lx) * f[..., y1, :][..., x0] + lx * f[..., y1, :][..., x1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def knot_coords64(k, n, size):
    k = [int(x) for x in k[:n]]
    out = np.empty(size)
    for j in range(size):
        i = n - 2
        for q in range(n - 1):
            if k[q] <= j < k[q + 1]:
                i = q
                break
        g0, g1 = -1 + 2 * i / (n - 1), -1 + 2 * (i + 1) / (n - 1)
        out[j] = g0 + (g1 - g0) * (j - k[i]) / max(k[i + 1] - k[i] - 1, 1)
    return out


def warp64(r, kx, ky, n):
    """r [C, H, W] float64 -> grid_sample (bilinear, zeros, align_corners = False) under the knots."""
    C, H, W = r.shape
    ix = ((knot_coords64(kx, n, W) + 1) * W - 1) / 2
    iy = ((knot_coords64(ky, n, H) + 1) * H - 1) / 2
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    lx, ly = ix - x0, iy - y0
    rp = np.pad(r, ((0, 0), (1, 1), (1, 1)))  # zeros outside: index i + 1 holds pixel i, for i = -1 .. size
    X0, X1, Y0, Y1 = x0 + 1, x0 + 2, y0 + 1, y0 + 2
    assert X0.min() >= 0 and X1.max() <= W + 1 and Y0.min() >= 0 and Y1.max() <= H + 1
    wy0, wy1 = (1 - ly)[:, None], ly[:, None]
    return (wy0 * (1 - lx) * rp[:, Y0][:, :, X0] + wy0 * lx * rp[:, Y0][:, :, X1]) + \
        (wy1 * (1 - lx) * rp[:, Y1][:, :, X0] + wy1 * lx * rp[:, Y1][:, :, X1])


def rays64(pose, h, fovy):
    """pose [4, 4] -> (rays_o, rays_d) [h, h, 3] float64."""
    pose = affine(pose)
    f = h / 2 / math.tan(math.radians(fovy) / 2)
    p = (np.arange(h) - h / 2 + 0.5) / f
    dirs = np.stack([np.broadcast_to(p[None, :], (h, h)), np.broadcast_to(-p[:, None], (h, h)), -np.ones((h, h))], -1)
    d = dirs @ pose[:3, :3].T
    d = d / np.sqrt(np.maximum((d * d).sum(-1, keepdims=True), 1e-20))
    return np.broadcast_to(pose[:3, 3], d.shape), d


def plucker64(pose, h, fovy):
    o, d = rays64(pose, h, fovy)
    return np.concatenate([np.cross(o, d), d], -1).transpose(2, 0, 1)


def views64(src, swap_rb, pose_in, knots, nknots, fovy, Vi, h, So, normalize=True):
    """src [B, V, Hs, Ws, 4] (the texel values as float32 holds them) -> input [B, Vi, 9, h, h], images_output
    [B, V, 3, So, So], masks_output [B, V, 1, So, So], float64."""
    x = np.asarray(src, np.float64).transpose(0, 1, 4, 2, 3)
    a = x[:, :, 3:4]
    rgb = x[:, :, [2, 1, 0]] if swap_rb else x[:, :, :3]
    c = rgb * a + (1 - a)
    B, V = c.shape[:2]
    inp = np.empty((B, Vi, 9, h, h))
    r = resize64(c[:, :Vi], h)
    for b in range(B):
        for v in range(Vi):
            n = 0 if knots is None else int(nknots[b, v])
            img = r[b, v] if n == 0 else warp64(r[b, v], knots[b, v, 0], knots[b, v, 1], n)
            inp[b, v, :3] = (img - MEAN[:, None, None]) / STD[:, None, None] if normalize else img
            inp[b, v, 3:] = plucker64(pose_in[b, v], h, fovy)
    return inp, resize64(c, So), resize64(a, So)
