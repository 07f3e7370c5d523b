"""Synthetic, seeded scenes for the ground detection tests: clouds as filter_node's front end leaves them (about one
point per 0.5 m voxel), sensor at the origin, the ground near z = -1.7.

A scene is a few thousand points: the smallest size at which the 512-point gates, the multi-ring neighbour walk (the
sparse far ground, poles) and more than one scoring workgroup (256 points each) are all exercised.
"""
import numpy as np

F32 = np.float32
GROUND_Z = -1.7


def _grid(rng, x0, x1, y0, y1, step, jitter):
    xs, ys = np.meshgrid(np.arange(x0, x1, step), np.arange(y0, y1, step), indexing="ij")
    p = np.stack([xs.ravel(), ys.ravel()], 1)
    return p + rng.uniform(-jitter, jitter, p.shape)


def scene(seed=0, radius=17.0, noise=0.03, clutter=0, walls=True, shuffle=True):
    """A noisy ground disc, three walls, poles and a ramp; `clutter` extra points scattered between the ground and the
    sensor's height (they survive the height clip: a low ground share for RANSAC).  Returns (N, 4) f32 x, y, z, intensity."""
    rng = np.random.default_rng(seed)
    g = _grid(rng, -radius, radius, -radius, radius, 0.5, 0.12)
    r = np.hypot(g[:, 0], g[:, 1])
    g = g[(r > 1.5) & (r < radius)]
    # far ground thins out, as a spinning lidar's rings do
    g = g[rng.uniform(0, 1, len(g)) < np.clip(1.6 - np.hypot(g[:, 0], g[:, 1]) / radius, 0.25, 1.0)]
    parts = [np.column_stack([g, GROUND_Z + rng.normal(0, noise, len(g))])]
    if walls:
        for (x0, y0, x1, y1) in ((-12, 9, 12, 9), (10, -8, 10, 8), (-14, -10, -6, -13)):
            L = np.hypot(x1 - x0, y1 - y0)
            t, z = np.meshgrid(np.arange(0, L, 0.5), np.arange(GROUND_Z + 0.25, GROUND_Z + 3.6, 0.5), indexing="ij")
            t, z = t.ravel(), z.ravel()
            w = np.column_stack([x0 + (x1 - x0) * t / L, y0 + (y1 - y0) * t / L, z])
            parts.append(w + rng.normal(0, 0.02, w.shape))
        for _ in range(9):  # poles
            c = rng.uniform(-13, 13, 2)
            z = np.arange(GROUND_Z + 0.3, GROUND_Z + 3.0, 0.5)
            parts.append(np.column_stack([np.full(len(z), c[0]), np.full(len(z), c[1]), z]) + rng.normal(0, 0.02, (len(z), 3)))
        rp = _grid(rng, 3.0, 9.0, -7.0, -3.0, 0.5, 0.1)  # a 25 degree ramp: inside the height clip, outside the normal filter
        parts.append(np.column_stack([rp, GROUND_Z + 0.05 + (rp[:, 0] - 3.0) * np.tan(np.radians(25.0)) + rng.normal(0, 0.02, len(rp))]))
    if clutter:
        c = rng.uniform(-radius, radius, (clutter, 2))
        parts.append(np.column_stack([c, rng.uniform(GROUND_Z + 0.3, 0.4, clutter)]))
    xyz = np.concatenate(parts)
    if shuffle:  # the front end's voxel order is not the construction order
        xyz = xyz[rng.permutation(len(xyz))]
    return np.column_stack([xyz, rng.uniform(0, 1, len(xyz))]).astype(F32)


def lattice(nx=40, ny=40, step=0.5, layers=(GROUND_Z, GROUND_Z + 1.0)):
    """Points on an exact lattice (every coordinate a multiple of `step` plus a constant representable in f32): every
    point has many neighbours at exactly equal distances, and many collinear triples.  A sparse layer above the height
    clip comes first, so the clipped cloud's indices are not the input's."""
    xs, ys = np.meshgrid(np.arange(nx) * step - nx * step / 2 + 0.25, np.arange(ny) * step - ny * step / 2 + 0.25, indexing="ij")
    parts = [np.column_stack([xs.ravel(), ys.ravel(), np.full(xs.size, z)]) for z in layers]
    parts[1] = parts[1][:: 7]  # a sparse second layer
    high = parts[0][:: 11].copy()
    high[:, 2] = 1.0
    parts.insert(0, high)
    xyz = np.concatenate(parts)
    return np.column_stack([xyz, np.linspace(0, 1, len(xyz))]).astype(F32)


def patch(n, seed=0, noise=0.01, extent=14.0, z=GROUND_Z):
    """Exactly n points of a noisy horizontal patch (every normal near vertical: all of them pass the normal filter)."""
    rng = np.random.default_rng(seed)
    xy = _grid(rng, -extent, extent, -extent, extent, 0.5, 0.1)
    xy = xy[np.hypot(xy[:, 0], xy[:, 1]) > 1.2][:n]
    assert len(xy) == n
    zz = np.full(n, z) if noise == 0 else z + rng.normal(0, noise, n)
    return np.column_stack([xy, zz, rng.uniform(0, 1, n)]).astype(F32)


def plane_and_clutter(n_plane, n_clutter, seed=0, z=GROUND_Z):
    """n_plane points exactly on z (f32) and n_clutter points at least 0.3 m off it, all inside the height clip."""
    rng = np.random.default_rng(seed)
    a = patch(n_plane, seed, noise=0.0, z=z)
    c = rng.uniform(-14, 14, (n_clutter, 2))
    cz = np.where(rng.uniform(0, 1, n_clutter) < 0.5, rng.uniform(z - 2.5, z - 0.3, n_clutter), rng.uniform(z + 0.3, 0.4, n_clutter))
    b = np.column_stack([c, cz, rng.uniform(0, 1, n_clutter)]).astype(F32)
    out = np.concatenate([a, b])
    return out[rng.permutation(len(out))]


def rotate_y(cloud, deg):
    """The cloud turned about the y axis by `deg` degrees (f64 rotation, rounded once)."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = np.asarray(cloud, np.float64).copy()
    out[:, :3] = out[:, :3] @ R.T
    return out.astype(F32)
