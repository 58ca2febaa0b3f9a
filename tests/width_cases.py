"""The cases of G20 (tests/golden/g20_width.npz): LYNXNet and the ConvNeXt aux decoder at widths that are not multiples of 32.
Shared by the generator (tests/golden/make_golden_width.py), the host tests and the GPU tests, so that all three build the same
seeded weights and inputs (diffsinger_amd/synth.py)."""

# tag: (in_dims, n_feats, backbone args, weight seed, [(B, T, t kind)])
LYNX_EVALS = {
    "c500": (128, 1, dict(num_layers=3, num_channels=500, expansion_factor=2, kernel_size=31, activation="PReLU",
                          strong_cond=False), 201, [(2, 70, "float"), (1, 33, "long")]),
    "c1000": (128, 1, dict(num_layers=2, num_channels=1000, expansion_factor=2, kernel_size=31, activation="PReLU",
                           strong_cond=True), 202, [(1, 40, "float")]),
    # inner = 270 and 2 * inner = 540: neither a multiple of 32
    "c90": (24, 2, dict(num_layers=2, num_channels=90, expansion_factor=3, kernel_size=7, activation="SiLU",
                        strong_cond=True), 203, [(2, 45, "float")]),
    "c6": (32, 1, dict(num_layers=2, num_channels=6, expansion_factor=1, kernel_size=5, activation="ReLU",
                       strong_cond=False), 204, [(2, 45, "long")]),
}

# one RectifiedFlow run: euler, 10 steps, injected x_T
SAMPLER = dict(in_dims=64, n_feats=1, args=dict(num_layers=2, num_channels=500, expansion_factor=2, kernel_size=31,
                                                activation="PReLU", strong_cond=True),
               wseed=205, bsz=2, t_len=50, steps=10, noise_seed=8000, cond_seed=8500)

# tag: (hidden, out_dims, decoder args, B, T, weight seed)
AUX = {
    "a500": (256, 64, dict(num_channels=500, num_layers=3, kernel_size=7, dropout_rate=0.1), 2, 40, 206),
    "a75": (192, 32, dict(num_channels=75, num_layers=3, kernel_size=7, dropout_rate=0.1), 3, 37, 207),
}


def eval_seeds(ci):
    """(x, cond, t) seeds of evaluation ci of a LYNX_EVALS case"""
    return 9000 + 10 * ci, 9001 + 10 * ci, 9002 + 10 * ci


def make_t(kind, bsz, seed):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "long":
        return rng.integers(0, 1000, size=(bsz,)).astype(np.int64)
    return (rng.random(size=(bsz,), dtype=np.float32) * np.float32(999.0)).astype(np.float32)
