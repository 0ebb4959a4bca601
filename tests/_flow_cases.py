"""TEST INFRASTRUCTURE ONLY: the case table of the voxel propagation chain, shared by tests/test_flow_reference.py (CPU: the
reference against the oracle) and tests/test_gpu_flow_chain.py (the kernels against the reference).

The long chains sit on both sides of the switch between the two launch forms of voxel_construct (csrc/cmax_flow.hip): one
k_voxel_chain_tiled launch while 4 (kVoxTileH + 2S)(kVoxTileW + 2S) sizeof(T) <= 60 KB, S = the longer of the two chains, one
k_flow_step_jobs launch per step beyond.  The three constants below restate kVoxTileH, kVoxTileW and the `lds <= 60 * 1024` test of
voxel_construct there: a change there has to be repeated here, and the long cases move with it."""
import numpy as np

VOX_TILE_H, VOX_TILE_W = 16, 32  # kVoxTileH, kVoxTileW (= kAdjTileH, kAdjTileW of cmax_flow_dual.h: the adjoint tiles)
VOX_LDS_BYTES = 60 * 1024        # the bound on the dynamic LDS of k_voxel_chain_tiled in voxel_construct

ITEMSIZE = {"float64": 8, "float32": 4}
# relative to the largest entry of the reference array (the bounds of test_random_leaf_operators_against_oracle)
TOL = {"float64": 1e-10, "float32": 2e-4}


def tiled_chain_limit(dtype):
    """The longest chain S the single-launch form still takes in `dtype`."""
    S = 0
    while 4 * (VOX_TILE_H + 2 * (S + 1)) * (VOX_TILE_W + 2 * (S + 1)) * ITEMSIZE[dtype] <= VOX_LDS_BYTES:
        S += 1
    return S


def chains(T, loc):
    """(backward, forward) chain lengths of a voxel of T bins."""
    t0 = 0 if loc == "first" else T // 2
    return t0, T - 1 - t0


# the smallest shapes at which each seam of the 16 x 32 tiles exists
SHAPES = [
    (1, 1),    # a single pixel
    (1, 40),   # a single row, two tile columns
    (37, 1),   # a single column, three tile rows
    (16, 32),  # exactly one tile
    (17, 33),  # four tiles, three of them one pixel wide or high
    (35, 70),  # 3 x 3 tiles, ragged last row and column
]
LONG_SHAPES = [(17, 33), (35, 70)]
FIELDS = ("rough", "smooth", "kinks")
SHORT_T = [(1, "middle"), (2, "first"), (2, "middle"), (7, "middle")]  # both ends, both parities


def long_T(dtype):
    """Chains S / S and S + 1 / S around bin t0 in the middle, S and S + 1 from the first bin: the last single-launch voxel and the
    first per-step one, in both placements."""
    S = tiled_chain_limit(dtype)
    out = [(2 * S + 1, "middle"), (2 * S + 2, "middle"), (S + 1, "first"), (S + 2, "first")]
    assert [max(chains(T, loc)) for T, loc in out] == [S, S + 1, S, S + 1]
    return out


def cases(dtype):
    """[(shape, T, t0 location, field)] for `dtype`."""
    out = [(shape, T, loc, field) for shape in SHAPES for T, loc in SHORT_T for field in FIELDS]
    out += [(shape, T, loc, field) for shape in LONG_SHAPES for T, loc in long_T(dtype) for field in FIELDS]
    return out


def case_id(case):
    (H, W), T, loc, field = case
    return f"{H}x{W}-T{T}{loc}-{field}"


def _round(a, dtype):
    return np.ascontiguousarray(a.astype(np.dtype(dtype)).astype(np.float64))


def field(name, shape, dtype):
    """[2,H,W] float64 array of amplitude 3 whose entries are exact in `dtype` (both sides see the same numbers)."""
    H, W = shape
    rng = np.random.default_rng([H, W, 11])
    rough = rng.uniform(-3.0, 3.0, (2, H, W))
    if name == "rough":
        return _round(rough, dtype)
    if name == "smooth":  # two low harmonics per channel, sign changes but no exact zero
        i, j = np.meshgrid(np.arange(H) / 16.0, np.arange(W) / 32.0, indexing="ij")
        u = 2.0 * np.sin(1.3 * i + 0.7 * j + 0.4) + np.cos(0.9 * j - 0.5 * i + 1.1)
        v = 2.0 * np.cos(0.8 * i - 1.1 * j + 2.0) + np.sin(1.7 * j + 0.3 * i - 0.6)
        return _round(np.stack([u, v]), dtype)
    assert name == "kinks"
    f = rough.copy()
    a, b = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    board = np.where((a + b) % 2 == 0, 1.0, -1.0)
    f[:, 2:8, 3:9] = (np.abs(f) * board)[:, 2:8, 3:9]  # a 6 x 6 checkerboard of signs
    f[0, min(VOX_TILE_H - 1, H - 1), :] = 0.0            # an all-zero row of u, the last row of the first tile (or of the image)
    f[1, :, min(VOX_TILE_W - 1, W - 1)] = 0.0            # an all-zero column of v, the last column of the first tile (or of the image)
    f[:, 14:19, 30:35] = 0.0                             # a block of exact zeros across both tile seams (rows 16, columns 32)
    return _round(f, dtype)


def directions(shape, T, dtype):
    """(dF [2,H,W], gV, dgV [T,2,H,W]): the tangent of the flow, a cotangent of the voxel and the tangent of that cotangent."""
    H, W = shape
    rng = np.random.default_rng([H, W, T, 12])
    return tuple(_round(rng.normal(size=s), dtype) for s in ((2, H, W), (T, 2, H, W), (T, 2, H, W)))
