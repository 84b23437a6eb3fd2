"""NumPy / plain Python restatement of sp_tsdf_mesh's rule (include/sp_hip.h), written from the rule and not from the kernel: marching
tetrahedra on the Kuhn split of every cell, vertices by a scan over ascending edge ids, faces by ascending (cell, tetrahedron, triangle),
every cycle oriented by the integer midpoint rule.  Test infrastructure only.  Also the volumes the tests cut (``sphere_volume`` ...)."""
import numpy as np

from tsdf_ref import node_centres

TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def _bits(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


def case_cycle(tet, negative, nx=2, ny=2):
    """The crossing edges of tetrahedron ``tet`` of the cell at node 0 of a lattice with ``nx`` x ``ny`` nodes per layer, when the local
    corners in ``negative`` (a set of 0 .. 3) are negative: a list of (lower corner, upper corner) in the rule's order -- a cycle that
    starts at the smallest edge id and whose midpoint triangle (q0, q1, q2) faces from the negative corners to the positive ones."""
    corners = TETS[tet]
    lin = lambda c: ((c >> 2) * ny + ((c >> 1) & 1)) * nx + (c & 1)
    crossing = []
    for i in range(4):
        for j in range(i + 1, 4):
            if (i in negative) != (j in negative):
                a, b = sorted((corners[i], corners[j]), key=lin)
                assert b & a == a and b != a                                           # b = a + offset: a lattice edge of type b - a
                crossing.append((lin(a) * 7 + (b - a) - 1, a, b))
    if not crossing:
        return []
    assert len(crossing) in (3, 4)
    crossing.sort()
    # walk the cycle from the smallest id: the next edge shares a corner with the current one (in a triangle every edge does)
    touch = lambda p, q: bool(set(p[1:]) & set(q[1:]))
    first, rest = crossing[0], crossing[1:]
    if len(rest) == 2:
        cycle = [first] + rest
    else:                                                                              # a quad: the edge opposite the first comes third
        opposite = [e for e in rest if not touch(e, first)]
        beside = [e for e in rest if touch(e, first)]
        assert len(opposite) == 1 and len(beside) == 2 and all(touch(e, opposite[0]) for e in beside)
        cycle = [first, beside[0], opposite[0], beside[1]]
    mid2 = [_bits(a) + _bits(b) for _, a, b in cycle]                                  # twice the midpoints: exact integers
    normal = np.cross(mid2[1] - mid2[0], mid2[2] - mid2[0])
    pos = [corners[k] for k in range(4) if k not in negative]
    neg = [corners[k] for k in range(4) if k in negative]
    direction = len(neg) * sum(_bits(c) for c in pos) - len(pos) * sum(_bits(c) for c in neg)          # npos nneg (centroid+ - centroid-)
    dot = int(normal @ direction)
    assert dot != 0
    if dot < 0:
        cycle = [cycle[0]] + cycle[:0:-1]
    return [(a, b) for _, a, b in cycle]


def orientation_table(nx=2, ny=2):
    """table[tet][case]: ``case`` has bit k set iff local corner k is negative."""
    return [[case_cycle(t, {k for k in range(4) if (case >> k) & 1}, nx, ny) for case in range(16)] for t in range(6)]


def mesh(tsdf, weight, colour, voxel, origin, min_weight=1.0):
    """tsdf, weight (nz,ny,nx) float32, colour (nz,ny,nx,3) float32 or None.  Returns dict(vertices (n,3) float32, colours (n,3) float32 or
    None, faces (F,3) int32, edge_ids (n,) int64 -- the lattice edge of every vertex)."""
    nz, ny, nx = tsdf.shape
    assert tsdf.dtype == np.float32 and weight.dtype == np.float32 and min(nx, ny, nz) >= 2
    with np.errstate(invalid='ignore'):
        valid = (weight >= np.float32(min_weight)) & np.isfinite(tsdf)
        negative = tsdf < 0
    N = nx * ny * nz
    crosses = np.zeros((N, 7), bool)
    upper = np.zeros((N, 7), np.int64)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    lin = ((iz * ny + iy) * nx + ix).reshape(-1)
    v_flat, n_flat = valid.reshape(-1), negative.reshape(-1)
    for e in range(1, 8):
        dx, dy, dz = e & 1, (e >> 1) & 1, e >> 2
        ok = ((ix + dx < nx) & (iy + dy < ny) & (iz + dz < nz)).reshape(-1)
        other = np.where(ok, lin + (dz * ny + dy) * nx + dx, 0)
        crosses[:, e - 1] = ok & v_flat & v_flat[other] & (n_flat != n_flat[other])
        upper[:, e - 1] = other
    flat = crosses.reshape(-1)
    edge_ids = np.nonzero(flat)[0]                                                     # ascending edge id = node * 7 + (bits - 1)
    vertex_of = np.full(N * 7, -1, np.int64)
    vertex_of[edge_ids] = np.arange(len(edge_ids))
    a, e = edge_ids // 7, edge_ids % 7 + 1
    b = upper.reshape(-1)[edge_ids]
    f = tsdf.reshape(-1).astype(np.float64)
    t = f[a] / (f[a] - f[b])
    pos = [node_centres(n, voxel, o) for n, o in zip((nx, ny, nz), origin)]
    idx = [a % nx, (a // nx) % ny, a // (nx * ny)]
    vertices = np.empty((len(edge_ids), 3), np.float32)
    for ax in range(3):
        pa = pos[ax][idx[ax]]
        pb = pos[ax][np.minimum(idx[ax] + ((e >> ax) & 1), len(pos[ax]) - 1)]
        vertices[:, ax] = (pa + t * (pb - pa)).astype(np.float32)
    colours = None
    if colour is not None:
        c = colour.reshape(-1, 3).astype(np.float64)
        colours = (c[a] + t[:, None] * (c[b] - c[a])).astype(np.float32)
    table = orientation_table(nx, ny)
    faces = []
    for cz in range(nz - 1):
        for cy in range(ny - 1):
            for cx in range(nx - 1):
                node = (cz * ny + cy) * nx + cx
                corner = [node + ((c >> 2) * ny + ((c >> 1) & 1)) * nx + (c & 1) for c in range(8)]
                if not any(n_flat[k] for k in corner) or all(n_flat[k] for k in corner):
                    continue
                for t_i, tet in enumerate(TETS):
                    if not all(v_flat[corner[c]] for c in tet):
                        continue
                    case = sum(1 << k for k in range(4) if n_flat[corner[tet[k]]])
                    q = [vertex_of[corner[lo] * 7 + (hi - lo) - 1] for lo, hi in table[t_i][case]]
                    assert all(v >= 0 for v in q)
                    if len(q) >= 3:
                        faces.append((q[0], q[1], q[2]))
                    if len(q) == 4:
                        faces.append((q[0], q[2], q[3]))
    return dict(vertices=vertices, colours=colours, faces=np.array(faces, np.int32).reshape(-1, 3), edge_ids=edge_ids)


# ---- what the tests ask of a mesh ---------------------------------------------------------------------------------------------------------
def edge_uses(faces):
    """{(low vertex, high vertex): [direction of every use: +1 = low -> high]}."""
    uses = {}
    for f in np.asarray(faces).tolist():
        for k in range(3):
            p, q = f[k], f[(k + 1) % 3]
            uses.setdefault((min(p, q), max(p, q)), []).append(1 if p < q else -1)
    return uses


# ---- the volumes ----------------------------------------------------------------------------------------------------------------------------
SPHERE = dict(dims=(12, 11, 10), voxel=0.05, origin=(-0.3, 0.2, 1.0), centre_nodes=(5.3, 4.9, 4.4), radius_voxels=3.3)


def sphere_centre():
    s = SPHERE
    return np.array([(c + 0.5) * np.float64(np.float32(s['voxel'])) + np.float64(np.float32(o)) for c, o in zip(s['centre_nodes'], s['origin'])])


def sphere_volume(hole=False):
    """12 x 11 x 10 nodes holding the distance to a sphere of radius 3.3 voxels centred off the lattice (negative inside), weight 2,
    colours a smooth function of the position.  ``hole``: a 3 x 3 x 3 block of nodes that straddles the surface has weight 0."""
    s = SPHERE
    nx, ny, nz = s['dims']
    p = [node_centres(n, s['voxel'], o) for n, o in zip(s['dims'], s['origin'])]
    c = sphere_centre()
    r = s['radius_voxels'] * np.float64(np.float32(s['voxel']))
    dist = np.sqrt((p[0][None, None, :] - c[0]) ** 2 + (p[1][None, :, None] - c[1]) ** 2 + (p[2][:, None, None] - c[2]) ** 2)
    tsdf = (dist - r).astype(np.float32)
    weight = np.full((nz, ny, nx), 2.0, np.float32)
    colour = np.stack(np.broadcast_arrays(0.5 + 0.4 * np.sin(7.0 * p[0])[None, None, :], 0.5 + 0.4 * np.cos(5.0 * p[1])[None, :, None],
                                          (p[2] - p[2][0])[:, None, None] / (p[2][-1] - p[2][0])), axis=-1).astype(np.float32)
    if hole:
        weight[3:6, 4:7, 7:10] = 0.0                                                   # (z, y, x): around the +x pole
    return dict(tsdf=tsdf, weight=weight, colour=colour, voxel=s['voxel'], origin=s['origin'], radius=r, centre=c)


def odd_volume():
    """5 x 4 x 3 nodes: an exact 0 on a node (positive), a NaN on a node of valid weight (invalid), one node of weight below the bound."""
    rng = np.random.default_rng(11)
    tsdf = rng.uniform(-1.0, 1.0, (3, 4, 5)).astype(np.float32)
    tsdf[1, 2, 2] = 0.0
    tsdf[0, 0, 0] = -0.0                                                               # (-0 < 0 is false: positive too)
    tsdf[1, 1, 3] = np.nan
    tsdf[2, 3, 1] = np.inf
    weight = np.full((3, 4, 5), 1.0, np.float32)
    weight[0, 2, 4] = 0.5
    colour = rng.uniform(0.0, 1.0, (3, 4, 5, 3)).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, colour=colour, voxel=0.25, origin=(0.5, -1.0, 2.0))


def minimum_volume():
    """2 x 2 x 2 nodes, one cell, corner 0 negative."""
    tsdf = np.array([-0.25, 0.5, 0.75, 0.5, 0.125, 1.0, 1.0, 1.0], np.float32).reshape(2, 2, 2)
    return dict(tsdf=tsdf, weight=np.ones((2, 2, 2), np.float32), colour=None, voxel=1.0, origin=(0.0, 0.0, 0.0))


_cache = {}


def reference(name, **kw):
    """The mesh of one of the volumes above, computed once."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        vol = dict(sphere=sphere_volume, holed=lambda: sphere_volume(hole=True), odd=odd_volume, minimum=minimum_volume)[name]()
        _cache[key] = (vol, mesh(vol['tsdf'], vol['weight'], vol['colour'], vol['voxel'], vol['origin'], **kw))
    return _cache[key]
