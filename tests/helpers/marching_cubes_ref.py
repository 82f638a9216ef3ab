"""numpy oracle of rnerf_marching_cubes_* (include/rnerf.h), exact: same vertices bit for bit, same triangles.

The case table is derived here from the face rule itself (it does not read csrc/mc_tables.h and shares no code with
tools/make_mc_tables.py): corners are bit x + 2y + 4z, edges 4 axis + a + 2 b.  marching_cubes() is vectorised over the active cells only.
"""
import functools
import itertools

import numpy as np


def edge_ends(e):
    """(base corner, far corner) of edge id e as (x, y, z) tuples."""
    axis, a, b = divmod(e, 4)[0], e % 2, (e // 2) % 2
    others = [d for d in range(3) if d != axis]
    c0 = [0, 0, 0]
    c0[others[0]], c0[others[1]] = a, b
    c1 = list(c0)
    c1[axis] = 1
    return tuple(c0), tuple(c1)


EDGE_OF = {frozenset(edge_ends(e)): e for e in range(12)}
EDGE_MID = np.array([(np.array(edge_ends(e)[0]) + np.array(edge_ends(e)[1])) / 2.0 for e in range(12)])


def bit(case, corner):
    return bool(case >> (corner[0] + 2 * corner[1] + 4 * corner[2]) & 1)


def face_cycle(d, side):
    """The four corners of face (axis d, side) in cyclic order."""
    u, v = [a for a in range(3) if a != d]
    out = []
    for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        c = [0, 0, 0]
        c[d], c[u], c[v] = side, cu, cv
        out.append(tuple(c))
    return out


def case_segments(case):
    segs = []
    for d, side in itertools.product(range(3), (0, 1)):
        cyc = face_cycle(d, side)
        s = [bit(case, c) for c in cyc]
        edge = [EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))] for i in range(4)]          # edge i joins corner i and i + 1
        cross = [i for i in range(4) if s[i] != s[(i + 1) % 4]]
        if len(cross) == 2:
            segs.append((edge[cross[0]], edge[cross[1]]))
        elif len(cross) == 4:
            for i in range(4):
                if s[i]:                                                                    # cut this solid corner off on its own
                    segs.append((edge[(i - 1) % 4], edge[i]))
    return segs


def case_loops(case):
    segs = case_segments(case)
    left = set(range(len(segs)))
    loops = []
    while left:
        start = min(min(segs[i]) for i in left)
        loop, cur = [start], start
        while True:
            i = next(i for i in sorted(left) if cur in segs[i])
            left.discard(i)
            cur = segs[i][0] if segs[i][1] == cur else segs[i][1]
            if cur == start:
                break
            loop.append(cur)
        p = EDGE_MID[loop]
        area = sum(np.cross(p[i], p[(i + 1) % len(loop)]) for i in range(len(loop))) / 2.0
        outward = np.zeros(3)
        for e in loop:
            c0, c1 = edge_ends(e)
            empty, sol = (c1, c0) if bit(case, c0) else (c0, c1)
            outward += np.array(empty, float) - np.array(sol, float)
        if float(np.dot(area, outward)) < 0:
            loop = loop[:1] + loop[1:][::-1]
        loops.append(loop)
    return sorted(loops, key=lambda l: l[0])


@functools.lru_cache(maxsize=None)
def table():
    """-> (tri int8 [256, 16] -1 padded, ntri int64 [256])."""
    tri = np.full((256, 16), -1, np.int8)
    ntri = np.zeros(256, np.int64)
    for case in range(256):
        k = 0
        for loop in case_loops(case):
            for i in range(1, len(loop) - 1):
                tri[case, k:k + 3] = (loop[0], loop[i], loop[i + 1])
                k += 3
        ntri[case] = k // 3
    tri.setflags(write=False); ntri.setflags(write=False)
    return tri, ntri


def marching_cubes(field, iso):
    """-> (verts float64 [V, 3] in index units, faces int32 [F, 3]) as include/rnerf.h specifies them."""
    f32 = np.ascontiguousarray(field, np.float32)
    gx, gy, gz = f32.shape
    n = f32.size
    iso = float(iso)
    f = f32.astype(np.float64)
    s = f > iso
    stride = (gy * gz, gz, 1)
    present = np.zeros((gx, gy, gz, 3), bool)
    present[:-1, :, :, 0] = s[:-1] != s[1:]
    present[:, :-1, :, 1] = s[:, :-1] != s[:, 1:]
    present[:, :, :-1, 2] = s[:, :, :-1] != s[:, :, 1:]
    flat = present.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1                   # vertex index of (node, axis) where present
    which = np.nonzero(flat)[0]
    node, axis = which // 3, which % 3
    ff = f.reshape(-1)
    f1 = ff[node]
    f2 = ff[node + np.asarray(stride)[axis]]
    with np.errstate(all="ignore"):
        t = (iso - f1) / (f2 - f1)
    t = np.where((t >= 0) & (t <= 1), t, 0.5)
    verts = np.stack(np.unravel_index(node, (gx, gy, gz)), 1).astype(np.float64)
    verts[np.arange(len(node)), axis] += t

    case = np.zeros((gx - 1, gy - 1, gz - 1), np.int64)
    for m in range(8):
        x, y, z = m & 1, (m >> 1) & 1, m >> 2
        case |= s[x:gx - 1 + x, y:gy - 1 + y, z:gz - 1 + z].astype(np.int64) << m
    tri, ntri = table()
    ci, cj, ck = np.nonzero((case != 0) & (case != 255))        # C order = cell-linear order
    cc = case[ci, cj, ck]
    cnode = (ci * gy + cj) * gz + ck
    cnt = ntri[cc]
    rep = np.repeat(np.arange(len(cc)), cnt)
    slot = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = tri[cc[rep][:, None], slot[:, None] * 3 + np.arange(3)[None, :]].astype(np.int64)      # [F, 3] edge ids
    eaxis, a, b = e >> 2, e & 1, (e >> 1) & 1
    off = np.where(eaxis == 0, a * stride[1] + b * stride[2], np.where(eaxis == 1, a * stride[0] + b * stride[2], a * stride[0] + b * stride[1]))
    owner = cnode[rep][:, None] + off
    assert flat[owner * 3 + eaxis].all()
    faces = vid[owner * 3 + eaxis].astype(np.int32)
    assert 3 * n <= 2 ** 31 - 1
    return verts, faces.reshape(-1, 3)


def num_crossed_edges(field, iso):
    s = np.asarray(field, np.float32).astype(np.float64) > float(iso)
    return int((s[:-1] != s[1:]).sum() + (s[:, :-1] != s[:, 1:]).sum() + (s[:, :, :-1] != s[:, :, 1:]).sum())


def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every directed edge occurs once and its opposite occurs once."""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    big = int(d.max()) + 1
    key, rkey = d[:, 0] * big + d[:, 1], d[:, 1] * big + d[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rkey))


def euler(verts, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, axis=1), axis=0)
    return len(verts) - len(und) + len(faces)


def signed_volume(verts, faces):
    p = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
