"""The frames both version-4 test files code (tests/test_tcbaac2d.py on the
host, tests/test_tcbaac2d_gpu.py on the GPU): name -> (u8 frame, (th, tw),
nclass).  Small on purpose; each takes another path of the tile scan."""
import numpy as np

TILE = (64, 64)


def _indices(rng, shape, scale):
    """Index-like symbols: mostly 128, Laplacian tails that cluster (a smooth envelope)."""
    H, W = shape[:2]
    env = 0.2 + (np.sin(np.arange(H)[:, None] / 9.0) * np.cos(np.arange(W)[None, :] / 13.0)) ** 2
    env = env.reshape(H, W, *([1] * (len(shape) - 2)))
    return np.clip(np.rint(128 + rng.laplace(0, scale, shape) * env), 0, 255).astype(np.uint8)


def cases():
    rng = np.random.Generator(np.random.PCG64(2024))
    return {
        "one_tile": (_indices(rng, (64, 64, 1), 3.0), TILE, 8),
        "cropped_3ch": (_indices(rng, (61, 77, 3), 2.0), TILE, 8),        # cropped both ways, unaligned rows
        "one_symbol": (np.array([[[200]]], np.uint8), TILE, 8),
        "one_row": (_indices(rng, (1, 130, 3), 4.0), TILE, 8),            # no upper neighbour anywhere
        "one_column": (_indices(rng, (130, 1, 1), 4.0), TILE, 8),         # no left neighbour anywhere
        "tiles_16x32": (_indices(rng, (128, 192, 3), 2.5), (16, 32), 5),  # non-square tiles, several classes
        "two_dims": (_indices(rng, (70, 50), 2.0), (32, 32), 3),          # (H, W): C = 1
        "all_128": (np.full((70, 70, 1), 128, np.uint8), TILE, 8),        # one context, 15 empty rows per class
        # every byte value, all 16 contexts, and tiles long enough (16384 symbols from a
        # prior total of ~8400) for the halving rule
        "uniform": (rng.integers(0, 256, (256, 256, 1), dtype=np.uint8), (128, 128), 2),
    }


def batch_frames():
    rng = np.random.Generator(np.random.PCG64(77))
    return np.stack([_indices(rng, (61, 77, 3), 1.5 + f) for f in range(3)])
