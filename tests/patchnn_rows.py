"""The (shape, variant) rows the GPU loss tests run the patch-NN search at (tests/test_gpu_loss.py), as one table: the CPU test asks the chooser
which instantiation each row launches and asserts that together they reach every one of the launch tables (tests/test_patchnn_choice_cpu.py);
the GPU test of the rows nobody ran before takes its parameters from NEW_ROWS.  A row: (Tx, Ty, H, W, ps, pt, stride, stridet, alpha, variant)."""


def frame(ps, s):
    """6 x 10 patch locations: the last group of a row is two locations wide"""
    return ps + 5 * s, ps + 9 * s


def rows_6x10(cases, variant):
    return [(tx, ty) + frame(ps, s) + (ps, 3, s, 1, alpha, variant) for tx, ty, ps, s, alpha in cases]


# test_patchnn_matrix_core_tile_counts (variant 6)
TILE_COUNT_ROWS = rows_6x10([(12, 100, 5, 2, 0.5), (62, 128, 7, 3, None), (50, 75, 11, 4, 0.5), (9, 17, 4, 1, 0.005), (82, 75, 5, 2, 0.5),
                             (82, 122, 11, 4, 0.5), (122, 182, 7, 4, None), (126, 190, 3, 2, 0.5), (30, 192, 5, 3, None)], 6)
# test_patchnn_kernel_variants_agree
VARIANT_ROWS = [(12, 20, 43, 51, ps, 3, s, 1, alpha, v) for v in (1, 2, 6, 0x806, 4) for ps, s, alpha in ((11, 4, 0.5), (7, 4, None), (3, 2, None))]
# test_alpha0_at_the_configured_clip_lengths (the default choice)
CLIP_LENGTH_ROWS = rows_6x10([(52, 75, 11, 4, 0.0), (52, 50, 11, 4, 0.0), (82, 122, 11, 4, 0.0), (122, 182, 7, 4, 0.0), (52, 75, 3, 2, 0.0)], 0)
# test_nn_and_fold_vs_oracle (the default choice)
ORACLE_ROWS = [(12, 20, 63, 71, 11, 3, 4, 1, 0.5, 0), (12, 20, 63, 71, 3, 3, 2, 1, None, 0), (3, 3, 11, 11, 11, 3, 4, 1, None, 0),
               (8, 5, 16, 20, 4, 2, 4, 2, 0.01, 0), (6, 30, 9, 9, 1, 1, 1, 1, None, 0)]

# test_patchnn_instantiations_no_other_test_reaches: (Tx, Ty, ps, stride, alpha, variant) -> the instantiation the row is there for,
# ("v6", tyt, nl, nw, xs) or ("v4", runsum, threads)
NEW_CASES = [
    ((60, 75, 5, 2, None, 6), ("v6", 5, 4, 8, 14)),
    ((30, 100, 5, 2, None, 6), ("v6", 8, 2, 4, 14)),
    ((30, 150, 5, 2, 0.5, 6), ("v6", 12, 1, 4, 16)),
    ((70, 150, 5, 2, None, 6), ("v6", 12, 1, 8, 14)),
    ((30, 192, 11, 4, 0.5, 0), ("v4", 1, 512)),
    ((82, 150, 5, 2, 0.5, 0), ("v4", 0, 1024)),
    ((30, 192, 5, 3, None, 0), ("v4", 0, 512)),       # (the tile-count test runs this clip on kernel 6 only)
]
NEW_ROWS = [rows_6x10([case[:5]], case[5])[0] for case, _ in NEW_CASES]

ALL_ROWS = TILE_COUNT_ROWS + VARIANT_ROWS + CLIP_LENGTH_ROWS + ORACLE_ROWS + NEW_ROWS

# the launch tables (csrc/vl3d_loss.hip launch_nn): 3 x 2 x 2 of kernel 6, five of kernel 4, kernel 2
LAUNCH_TABLE = ({("v6", tyt, nl, nw, xs) for tyt, nl in ((5, 4), (8, 2), (12, 1)) for nw in (4, 8) for xs in (14, 16)} |
                {("v4", 1, 256), ("v4", 0, 256), ("v4", 1, 512), ("v4", 0, 512), ("v4", 0, 1024)} | {("v2",)})


def loss_desc(row):
    """the descriptor utils_vid._loss_desc builds for dense [3, T, H, W] videos of this row"""
    from videoloop3d_amd import _lib as L
    Tx, Ty, H, W, ps, pt, s, st, alpha, variant = row
    d = L.LossDesc()
    d.Tx, d.Ty, d.H, d.W, d.ps, d.pt, d.stride, d.stridet = Tx, Ty, H, W, ps, pt, s, st
    d.use_alpha, d.alpha = (0, 0.0) if alpha is None else (1, float(alpha))
    d.x_sc, d.x_st, d.x_sr, d.y_sc, d.y_st, d.y_sr = Tx * H * W, H * W, W, Ty * H * W, H * W, W
    d.variant = variant
    return d


def instantiation(c):
    """an L.NNChoice as a member of LAUNCH_TABLE"""
    return {6: ("v6", c.tyt, c.nl, c.nw, c.xs), 4: ("v4", c.runsum, c.threads), 2: ("v2",)}[c.kernel]
