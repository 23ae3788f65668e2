"""The tile grids around the limits of the forward and backward (plain numpy, no GPU): the case table, the scene builders
and each case's preconditions, checked on the oracle's lists by tests/test_tile_grid_cpu.py so that a case which no
longer exercises its target fails on the CPU before anyone takes it to a GPU (tests/test_tile_grid_gpu.py).

With T = ceil(W/16) ceil(H/16) tiles:
  bin_scatter_kernel scans the tile totals `per` = ceil(T / 1024) tiles per thread (at most 16);
  preprocess_kernel / bin_scatter_kernel take 4 T bytes of dynamic LDS, 64 KB at kBinMaxTiles = 16 384;
  tile_order_kernel's second slot per thread is live above 8 192 tiles; the segment tables walk the tiles 1024 at a time;
  above 16 384 tiles the forward takes the radix route whatever the context was told, with no tile order, no split lists,
  no compact lists, and a radix key of tile_bits(T) bits (17 from 65 537 tiles on).
"""
import numpy as np

TILE = 16
BIN_THREADS = 1024       # gs_common.h: kBinThreads
BIN_MAX_TILES = 16384    # gs_common.h: kBinMaxTiles
SEG_SPLIT_MIN = 1488     # gs_render.h: kSegSplitMin

# name: (ntx, nty, W, H, l_max, gaussians, what the grid hits)
GRIDS = {
    "t1024": (32, 32, 512, 512, 1, 20000, "per = 1, full"),
    "t1025": (41, 25, 656, 400, 1, 20000, "per = 2"),
    "t4097": (17, 241, 272, 3856, 1, 20000, "per = 5, tall"),
    # 8 193 = 3 x 2731 has no other factors, and on an image 48 pixels wide the generator's splats are thousands of pixels
    # long (5.5 M instances); 91 x 91 is the nearest grid with the same properties that the generator fills like the others
    "t8281": (91, 91, 1456, 1456, 1, 20000, "per = 9; second slot of tile_order_kernel; ninth trip of the segment tables"),
    "t16383": (127, 129, 2025, 2057, 1, 20000, "both edges ragged; T % 8 = 7"),
    "t16384": (128, 128, 2048, 2048, 1, 20000, "the limit itself"),
    "t16384_strip": (1024, 16, 16384, 256, 1, 20000, "the limit as a strip"),
    "t16385": (145, 113, 2320, 1808, 1, 20000, "first grid past the limit"),
    "t16512": (129, 128, 2064, 2048, 1, 20000, "past the limit"),
    "t16400_strip": (1025, 16, 16400, 256, 1, 20000, "strip past the limit"),
    "t65792": (257, 256, 4112, 4096, 0, 30000, "tile ids >= 65 536; key width 17"),
}
SMALL_VIEW = (640, 360)  # the small view of the mixed-size sequence (920 tiles)


def per_of(T):
    return -(-T // BIN_THREADS)


def tile_bits(T):
    """Bits of the radix route's tile key: the smallest b with T <= 2^b (at least 1)."""
    b = 1
    while (1 << b) < T:
        b += 1
    return b


def _place(params, cam, rows, u, v, z):
    """Move gaussians `rows` to the pixel positions (u, v) at depths z (identity pose) and make them about one pixel."""
    W, H = cam["width"], cam["height"]
    params["xyz"][rows, 0] = (u - W / 2.0) * z / cam["fx"]
    params["xyz"][rows, 1] = (v - H / 2.0) * z / cam["fy"]
    params["xyz"][rows, 2] = z
    params["scale"][rows] = np.log(0.004)


def hot_tile(W, H):
    """The tile the skewed and long-list scenes fill: in the last full tile row, three tiles before its end."""
    ntx = (W + TILE - 1) // TILE
    ty = H // TILE - 1
    tx = max(0, min(ntx - 1, W // TILE - 1) - 3)
    return tx, ty


def build_scene(scene, W, H, L, N, kind="plain", hole=None):
    """(params, camera) of a case.  kind: "plain" -- make_gaussians with three gaussians placed in the last tile (at
    20 000 gaussians on 16 384 tiles a given tile is empty one time in four); "skewed" -- 300 one-pixel gaussians in one
    tile near the end of the grid as well, so that the longest list is far above three times the average; "long" -- 2 000
    of them, a list beyond kSegSplitMin.  The one-pixel gaussians take five distinct depths.  hole = (tx0, tx1, ty0, ty1):
    the gaussians that project into those tiles are moved behind the camera, which leaves a run of empty tiles."""
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, 0)
    rng = np.random.default_rng(23)
    # the last tile (partial when the edges are ragged): three ordinary gaussians around a pixel inside it
    lu, lv = W - 1 - min(4, (W - 1) % TILE), H - 1 - min(4, (H - 1) % TILE)
    rows = np.arange(3)
    z = np.float64([3.0, 5.0, 8.0])
    params["xyz"][rows, 0] = (lu + np.float64([-1, 0, 1]) - W / 2.0) * z / cam["fx"]
    params["xyz"][rows, 1] = (lv + np.float64([0, -1, 1]) - H / 2.0) * z / cam["fy"]
    params["xyz"][rows, 2] = z
    k = dict(plain=0, skewed=300, long=2000)[kind]
    if k:
        tx, ty = hot_tile(W, H)
        rows = np.arange(100, 100 + k)
        u = TILE * tx + 4.0 + 8.0 * rng.random(k)
        v = TILE * ty + 4.0 + 8.0 * rng.random(k)
        _place(params, cam, rows, u, v, rng.choice(np.float64([2.5, 3.25, 4.0, 7.5, 11.0]), k))
        params["opacity"][rows] = rng.choice([-5.0, -4.0, -3.0, -1.0], size=k, p=[0.5, 0.3, 0.15, 0.05])
    if hole is not None:
        tx0, tx1, ty0, ty1 = hole
        x, y, zz = params["xyz"][:, 0].astype(np.float64), params["xyz"][:, 1].astype(np.float64), params["xyz"][:, 2]
        u = x / zz * cam["fx"] + W / 2.0
        v = y / zz * cam["fy"] + H / 2.0
        inside = (u >= TILE * tx0) & (u < TILE * tx1) & (v >= TILE * ty0) & (v < TILE * ty1)
        params["xyz"][inside, 2] *= -1.0
    return params, cam


def grid_scene(scene, name, kind="plain"):
    ntx, nty, W, H, L, N, _ = GRIDS[name]
    hole = (40, 200, 99, 102) if name == "t65792" else None  # three tile rows: the middle one stays empty
    return build_scene(scene, W, H, L, N, kind, hole)


def grad_image(scene, W, H):
    """scene.make_grad_image; beyond 8 M pixels a sixteenth of the rows, repeated (the generator needs seconds there)."""
    if W * H <= (8 << 20) or H % 16:
        return scene.make_grad_image(W, H)
    return np.tile(scene.make_grad_image(W, H // 16), (16, 1, 1)) / np.float32(16.0)


def oracle_forward(orc, scene, params, cam, L, threads=16):
    c = scene.CONFIG
    return orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=threads)


def longest_empty_run(lens):
    """Length of the longest run of consecutive empty tiles."""
    empty = np.concatenate([[0], (np.asarray(lens) == 0).astype(np.int64), [0]])
    edges = np.flatnonzero(np.diff(empty))
    return int((edges[1::2] - edges[::2]).max()) if len(edges) else 0


def check_preconditions(name, kind, ref):
    """Asserts on an oracle forward that the case exercises what the table says.  Returns the figures."""
    ntx, nty, W, H, L, N, _ = GRIDS[name]
    T = ntx * nty
    assert ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE) == (ntx, nty)
    ranges = np.asarray(ref["ranges"])
    assert len(ranges) == T + 1
    lens = np.diff(ranges).reshape(nty, ntx)
    S = int(ranges[-1])
    assert S == len(ref["sorted"])
    assert lens[-1, -1] > 0, "the last tile is empty"
    assert lens[-1].any() and lens[:, -1].any(), "the last tile row / column is empty"
    per = per_of(T)
    assert lens.reshape(-1)[BIN_THREADS * (per - 1):].any(), "no tile in the last thread's share of the scan"
    flat = lens.reshape(-1)
    if T > 8192:
        assert flat[8192:].any()          # tile_order_kernel's second slot, the tables' ninth trip
    if T > 65536:
        assert flat[65536:].any(), "no list with a tile id of 17 bits"
        assert tile_bits(T) == 17
        assert longest_empty_run(flat) >= 64, "no run of 64 empty tiles"
    longest = int(flat.max())
    if kind == "plain":
        assert longest <= SEG_SPLIT_MIN
    if kind == "skewed":
        assert longest <= SEG_SPLIT_MIN and longest * T > 3 * S, "the tile order would not pay"
    if kind == "long":
        assert longest > SEG_SPLIT_MIN, "no list beyond kSegSplitMin"
        assert int(flat.argmax()) > T - 8 * ntx, "the long list is not near the end of the grid"
    if kind != "plain":
        tx, ty = hot_tile(W, H)
        assert int(flat.argmax()) == ty * ntx + tx
    assert S < 768 * T  # (the dense radix branch is not what these cases are about)
    return dict(T=T, per=per, S=S, M=int(ref["num_culled"]), longest=longest, empty=int((flat == 0).sum()),
                empty_run=longest_empty_run(flat))


# which (grid, kind) pairs the GPU tests use: every grid plain; the skewed scene (tile order) and the long-list scene
# (segment tables) at 8 281 tiles -- the one grid on which tile_order_kernel's second slot and the tables' ninth trip are
# PARTLY live (per_xcd = 1036: twelve threads of the second slot; 89 tiles in the ninth trip) -- and around the limit
ORDER_GRIDS = ("t8281", "t16383", "t16384", "t16385")
SEGMENT_GRIDS = ("t8281", "t16384", "t16385")
CASES = ([(name, "plain") for name in GRIDS] + [(name, "skewed") for name in ORDER_GRIDS] +
         [(name, "long") for name in SEGMENT_GRIDS])


def check_hot_tile_is_in_the_partial_slots(name):
    """At 8 281 tiles the skewed / long-list tile lies behind tile 8 192 (the ninth trip of the segment tables) and in its
    XCD run's second slot (offset >= 1024 in a run of per_xcd = 1036 tiles)."""
    ntx, nty, W, H = GRIDS[name][:4]
    T = ntx * nty
    tx, ty = hot_tile(W, H)
    t = ty * ntx + tx
    per_xcd = (T + 7) >> 3
    assert 1024 < per_xcd < 2048 and t >= 8192 and t % per_xcd >= 1024, (t, per_xcd)
    return t, per_xcd


def small_long_scene(scene):
    """The 640x360 view with the long-list scene (the mixed-size sequence renders it between two large views)."""
    W, H = SMALL_VIEW
    return build_scene(scene, W, H, 1, 20000, "long")


# ---- further scenes of the GPU file
EMPTY_TAIL_GRIDS = ("t16384", "t16512")


def empty_tail_scene(scene, name):
    """A grid's plain scene with everything that projects into the last four tile rows (and beside them) moved behind
    the camera: the last tile rows hold no list."""
    ntx, nty, W, H, L, N, _ = GRIDS[name]
    return build_scene(scene, W, H, L, N, hole=(-8, ntx + 8, nty - 4, nty + 8))


def check_empty_tail(name, ref, full_ref):
    ntx = GRIDS[name][0]
    lens = np.diff(ref["ranges"])
    assert (lens[-ntx:] == 0).all(), "the last tile row is not empty"
    assert longest_empty_run(lens) >= ntx
    assert len(ref["sorted"]) < len(full_ref["sorted"])  # (a forward of the full scene leaves larger ranges behind)


ABSGRAD_GAUSSIANS = 6000  # the float64 absgrad reference walks every tile's pixels per list position: 7 s for 20 000


def absgrad_scene(scene):
    """The 16 512-tile grid with 6 000 gaussians."""
    _, _, W, H, L, _, _ = GRIDS["t16512"]
    return build_scene(scene, W, H, L, ABSGRAD_GAUSSIANS)


def check_absgrad_scene(ref):
    lens = np.diff(ref["ranges"])
    assert len(lens) == 16512 and lens[-1] > 0 and lens[BIN_MAX_TILES:].any()


# (ntx, nty, tiles left empty at the end) of the stand-alone binning operator's cases
BAND_GRIDS = [(16384, 1, 0), (1, 16384, 0), (16385, 1, 0), (128, 128, 0), (129, 128, 0), (129, 128, 5 * 129), (257, 256, 0),
              (1, 1, 0), (2, 1, 0), (3, 1, 0)]


def band_scene(ntx, nty, empty_tail=0):
    """(uv, xyz_c, radius) of the binning operator's inputs: 20 000 gaussians (200 on grids of at most three tiles) over
    an ntx x nty grid, with radii from one pixel to a few tiles, random rotations and few distinct depths; a third of the
    grid's tiles stay empty in runs (the gaussians avoid every third block of 96 tiles of a strip, every third band of
    eight tile rows of a square grid); empty_tail: nothing in that many tiles at the end."""
    M = 20000 if ntx * nty > 3 else 200
    rng = np.random.default_rng(ntx * 7 + nty)
    T = ntx * nty
    tile = rng.integers(0, T, M)
    if ntx > 1 and nty >= 24:  # whole bands of eight tile rows (the largest radius reaches two tiles into a band)
        row = tile // ntx
        tile = np.where((row // 8) % 3 == 1, np.minimum(tile + 8 * ntx, T - 1), tile)
    elif T >= 288:
        tile = np.where((tile // 96) % 3 == 1, np.minimum(tile + 96, T - 1), tile)
    tile[:3] = (0, T - 1, T // 2)
    if empty_tail:
        tile = np.minimum(tile, T - 1 - empty_tail)
    u = 16.0 * (tile % ntx) + 16.0 * rng.random(M)
    v = 16.0 * (tile // ntx) + 16.0 * rng.random(M)
    uv = np.stack([u, v], 1).astype(np.float32)
    xyz = np.zeros((M, 3), np.float32)
    xyz[:, 2] = rng.choice(np.float32([0.5, 1.25, 2.0, 7.5, 31.0, 40.5, 63.0]), M)
    major = np.ceil(rng.choice([1.0, 3.0, 9.0, 30.0], M, p=[0.4, 0.3, 0.2, 0.1]))
    minor = np.ceil(major * rng.uniform(0.3, 1.0, M))
    ang = rng.uniform(0, np.pi, M)
    radius = np.stack([major, minor, np.sin(ang), np.cos(ang)], 1).astype(np.float32)
    return uv, xyz, radius


def check_band_scene(ntx, nty, empty_tail, ranges):
    """On the oracle's ranges: first tile filled; last tile filled, or the last tile row empty; a run of 64 empty tiles."""
    lens = np.diff(ranges)
    assert len(lens) == ntx * nty and lens[0] > 0
    if empty_tail:
        assert (lens[-ntx:] == 0).all() and lens.any()
    else:
        assert lens[-1] > 0
    if ntx * nty > 3:
        assert longest_empty_run(lens) >= 64
    if ntx * nty > 65536:
        assert lens[65536:].any()
