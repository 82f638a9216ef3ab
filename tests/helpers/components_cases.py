"""The input grids of the connected-component tests (uint8 [X,Y,Z], non-zero = solid), shared by tests/test_components_host.py and
tests/test_gpu_components.py.  Everything is seeded or closed-form."""
import numpy as np


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def checkerboard(n=9):
    x, y, z = np.indices((n, n, n))
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def snake(shape=(5, 41, 67)):
    """A one-voxel-wide path in the plane x = 2: every other row of z, joined alternately at either end. -> (grid, length)."""
    X, Y, Z = shape
    g = np.zeros(shape, np.uint8)
    rows = list(range(0, Y, 2))
    for r, y in enumerate(rows):
        g[2, y, :] = 1
        if y + 2 < Y:
            g[2, y + 1, Z - 1 if r % 2 == 0 else 0] = 1
    return g, int(g.sum())


def pair_lattice(n=34, second=(1, 1, 1)):
    """Voxels (3i, 3j, 3k) and (3i, 3j, 3k) + second."""
    g = np.zeros((n, n, n), np.uint8)
    a = np.arange(0, n - 1, 3)
    ii, jj, kk = np.meshgrid(a, a, a, indexing="ij")
    g[ii, jj, kk] = 1
    g[ii + second[0], jj + second[1], kk + second[2]] = 1
    return g


def small_cases():
    """name -> grid: every case of the issue but the 160^3 one."""
    cases = {}
    for shape in ((33, 20, 70), (17, 9, 130)):
        for p in (0.32, 0.5):
            cases["bernoulli_%dx%dx%d_p%g" % (shape + (p,))] = bernoulli(shape, p, 1000 + shape[0] + int(100 * p))
    cases["one_solid"] = np.ones((1, 1, 1), np.uint8)
    cases["one_empty"] = np.zeros((1, 1, 1), np.uint8)
    cases["line_1x7x300"] = bernoulli((1, 7, 300), 0.6, 7)
    cases["cube_2x2x2"] = bernoulli((2, 2, 2), 0.5, 8)
    cases["all_solid"] = np.ones((9, 10, 70), np.uint8)
    cases["all_empty"] = np.zeros((9, 10, 70), np.uint8)
    cases["checkerboard"] = checkerboard(9)
    cases["snake"] = snake()[0]
    cases["corner_pairs"] = pair_lattice(34, (1, 1, 1))
    cases["edge_pairs"] = pair_lattice(34, (1, 1, 0))
    return cases


def ball(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


def shell_scene():
    """A hollow shell (radius 10 +- 1.5 in 32^3) with one floater inside the cavity, one outside and one touching the border.
    -> (grid, shell bool, cavity bool)."""
    shape, c = (32, 32, 32), (16, 16, 16)
    shell = ball(shape, c, 11.5) & ~ball(shape, c, 8.5)
    cavity = ball(shape, c, 8.5)
    g = shell.astype(np.uint8)
    g[15:17, 15:17, 15:17] = 1          # inside the cavity
    g[2:4, 2:4, 2:4] = 1                # outside, free
    g[0:2, 28:30, 14:16] = 1            # outside, on the face x = 0
    return g, shell, cavity


def torus(shape=(32, 32, 14), R=9.0, r=3.2):
    x, y, z = np.indices(shape).astype(np.float64)
    x -= (shape[0] - 1) / 2; y -= (shape[1] - 1) / 2; z -= (shape[2] - 1) / 2
    return (((np.sqrt(x * x + y * y) - R) ** 2 + z * z) <= r * r).astype(np.uint8)


def box_with_cavity(channel):
    """A solid 9^3 box inside 13^3 with a 3^3 cavity; channel None: closed; "straight": a one-voxel channel along -x to the border;
    "diagonal": a channel whose steps are only diagonal (26-adjacent, not 6-adjacent)."""
    g = np.zeros((13, 13, 13), np.uint8)
    g[2:11, 2:11, 2:11] = 1
    g[5:8, 5:8, 5:8] = 0
    if channel == "straight":
        g[0:5, 6, 6] = 0
    elif channel == "diagonal":
        for k, x in enumerate(range(4, 1, -1)):          # (4, 7, 6), (3, 6, 6), (2, 7, 6): each shares only an edge with the one before
            g[x, 6 + (k + 1) % 2, 6] = 0
    return g
