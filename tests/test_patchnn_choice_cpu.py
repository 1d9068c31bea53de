"""Which kernel the patch-NN search and the vote-fold run, asked of the library without a GPU (vl3d_patchnn_choice / vl3d_vote_fold_choice: the
functions the entry points call, csrc/vl3d_patchnn_choice.h): one named case per promise of include/vl3d.h and docs/kernels/K3_patch_nn.md, a
sweep of invariants over sizes x patch settings x variants x entries, the scratch size against the values recorded before it was computed
from the shared patch grid, the chooser's header on its own under plain g++ and the host sanitizers, and the instantiations the GPU loss
tests' shapes reach."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import patchnn_rows as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, 1, 3
KIB = 1024


@pytest.fixture(scope="module")
def UV():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import utils_vid
    return utils_vid


def desc_of(tx, ty, ps, s, alpha, variant, H=None, W=None, pt=3, st=1):
    """H, W default to 6 x 10 patch locations"""
    h, w = PR.frame(ps, s)
    return PR.loss_desc((tx, ty, H or h, W or w, ps, pt, s, st, alpha, variant))


def nn(UV, *a, entry="plain", has_scratch=True, x_pitch=None, x_frames=None, y_pitch=None, **kw):
    d = desc_of(*a, **kw)
    rc, c = UV.patchnn_choice(d, entry, has_scratch, d.W if x_pitch is None else x_pitch, d.Tx if x_frames is None else x_frames,
                              d.W if y_pitch is None else y_pitch)
    return rc, c


H720, W720 = 719, 1279          # the 720p frame trimmed to both shipped patch grids ((ps, stride) = (11, 4) and (3, 2))

# (Tx, Ty, ps, stride, alpha, variant) -> (kernel, instantiation, ch (kernel 6), lds_bytes)
NAMED = [
    ((50, 75, 11, 4, .5, 6), (6, (5, 4, 4, 16), 1, 45104)),
    ((12, 100, 5, 2, .5, 6), (6, (8, 2, 4, 16), 3, 55232)),
    ((62, 128, 7, 3, None, 6), (6, (8, 2, 8, 14), 1, 76928)),
    ((82, 75, 5, 2, .5, 6), (6, (5, 4, 8, 16), 2, 52368)),
    ((82, 122, 11, 4, .5, 6), (6, (8, 2, 8, 16), 1, 73952)),
    ((122, 182, 7, 4, None, 6), (6, (12, 1, 8, 16), 1, 94672)),
    ((126, 190, 3, 2, .5, 6), (6, (12, 1, 8, 16), 1, 101840)),
    ((30, 192, 5, 3, None, 6), (6, (12, 1, 4, 14), 1, 56640)),
    ((30, 192, 5, 3, None, 0), (4, (0, 512), None, 37632)),          # one location per wave loses to kernel 4's four locations
    ((82, 150, 11, 4, .5, 0), (4, (0, 1024), None, 65136)),          # ... 82 x 150 frames: the measured case; no running sums at 1024 threads
    ((30, 192, 11, 4, .5, 0), (4, (1, 512), None, 61824)),           # running sums: ps >= 2 stride
]


@pytest.mark.parametrize("case,want", NAMED, ids=[str(c[0]) for c in NAMED])
def test_named_choice(UV, case, want):
    rc, c = nn(UV, *case)
    kernel, inst, ch, lds = want
    assert rc == OK and c.kernel == kernel and c.lds_bytes == lds
    if kernel == 6:
        assert ((c.tyt, c.nl, c.nw, c.xs), c.ch, c.threads, c.scratch_layout) == (inst, ch, 64 * inst[2], 1)
    else:
        assert ((c.runsum, c.threads), c.scratch_layout) == (inst, 2)


def test_long_clips_and_refusals(UV):
    rc, c = nn(UV, 130, 200, 5, 2, None, 0)                       # beyond kernel 6's x range and kernel 4's 1024 tiles
    assert (rc, c.kernel, c.threads, c.scratch_layout) == (OK, 2, 256, 2) and 0 < c.kc <= 75 and c.lds_bytes <= 150 * KIB
    assert nn(UV, 130, 75, 5, 2, None, 6)[0] == EINVAL            # variant 6 outside its range
    assert nn(UV, 150, 260, 5, 2, None, 0)[0] == EINVAL           # the frame-pair matrix does not fit LDS
    assert nn(UV, 50, 75, 5, 2, None, 3)[0] == EINVAL             # the removed fp32 matrix-core kernel
    assert nn(UV, 50, 75, 5, 2, None, 0x10)[0] == EINVAL          # check_loss: ablation bits
    assert nn(UV, 51, 75, 5, 2, None, 0, pt=2, st=2)[0] == EINVAL     # check_loss: x not trimmed to the patch grid
    for variant in (1, 2, 5, 7, 15):                              # 1 keeps its meaning with scratch: kernel 2; so does every unnamed value
        assert nn(UV, 50, 75, 5, 2, None, variant)[1].kernel == 2
    out = UV.L.NNChoice()
    assert UV.L.lib().vl3d_patchnn_choice(desc_of(50, 75, 5, 2, None, 0), 3, 1, 0, 0, 0, UV.L.C.byref(out)) == EINVAL
    assert UV.L.lib().vl3d_patchnn_choice(desc_of(50, 75, 5, 2, None, 0), 0, 1, 0, 0, 0, None) == EINVAL


def test_null_scratch_is_refused_by_name(UV):
    """vl3d_patchnn without scratch ran the strided-staging kernel, whatever desc->variant said; that kernel is gone"""
    for variant in (0, 1, 2, 4, 6):
        rc, c = nn(UV, 50, 75, 5, 2, None, variant, has_scratch=False)
        assert rc == EINVAL and c.kernel == 0
    assert b"vl3d_patchnn_scratch_bytes" in UV.L.lib().vl3d_last_error()
    assert nn(UV, 50, 75, 5, 2, None, 0, entry="prepared", has_scratch=False)[0] == EINVAL       # x's gram16 copy lives there
    assert nn(UV, 50, 75, 5, 2, None, 0, entry="grams", has_scratch=False)[0] == OK              # no scratch by design


def test_the_shipped_720p_views(UV):
    rc, c = nn(UV, 52, 75, 11, 4, 0.0, 0, H=H720, W=W720)
    assert (rc, c.kernel, (c.tyt, c.nl, c.nw, c.xs), c.ch, c.lds_bytes) == (OK, 6, (5, 4, 4, 16), 1, 45808)
    rc, c = nn(UV, 52, 75, 3, 2, None, 0, H=H720, W=W720)
    assert (rc, c.kernel, (c.tyt, c.nl, c.nw, c.xs), c.ch, c.lds_bytes) == (OK, 6, (5, 4, 4, 14), 4, 49872)
    for entry in ("prepared", "grams"):                           # the training loop's entries: the same instantiations
        c = nn(UV, 52, 75, 11, 4, 0.0, 0, H=H720, W=W720, entry=entry, x_pitch=1280, x_frames=52, y_pitch=1280)[1]
        assert (c.kernel, c.tyt, c.nl, c.nw, c.xs, c.lds_bytes) == (6, 5, 4, 4, 16, 45808)


def test_the_per_wave_epilogue_boundary(UV):
    """xs = 14: four waves hold 4 x 14 + 2 = 58 frames of x; one more takes eight waves.  With alpha the tiles abut (xs 16): four waves to 64."""
    inst = lambda c: (c.kernel, c.nw, c.xs)
    assert inst(nn(UV, 58, 75, 5, 2, None, 0)[1]) == (6, 4, 14) and inst(nn(UV, 59, 75, 5, 2, None, 0)[1]) == (6, 8, 14)
    assert inst(nn(UV, 58, 75, 5, 2, .5, 0)[1]) == (6, 4, 16) and inst(nn(UV, 59, 75, 5, 2, .5, 0)[1]) == (6, 4, 16)
    assert inst(nn(UV, 64, 75, 5, 2, .5, 0)[1]) == (6, 4, 16) and inst(nn(UV, 65, 75, 5, 2, .5, 0)[1]) == (6, 8, 16)
    assert inst(nn(UV, 50, 75, 5, 2, None, 0x806)[1]) == (6, 4, 16)      # bit 11: the workgroup-wide epilogue also without alpha
    assert inst(nn(UV, 50, 75, 5, 2, None, 6, pt=2, st=2)[1]) == (6, 4, 16)


def test_prepared_entries_have_kernel_6_or_nothing(UV):
    for entry in ("prepared", "grams"):
        assert nn(UV, 50, 75, 5, 2, None, 4, entry=entry)[0] == EINVAL
        assert nn(UV, 50, 75, 5, 2, None, 2, entry=entry)[0] == EINVAL
        assert nn(UV, 50, 75, 5, 2, None, 6, entry=entry)[1].kernel == 6
        assert nn(UV, 130, 75, 5, 2, None, 0, entry=entry)[0] == EUNSUPPORTED      # x beyond 128 frames
        assert nn(UV, 50, 200, 5, 2, None, 0, entry=entry)[0] == EUNSUPPORTED      # y beyond 192 frames
        rc, c = nn(UV, 30, 192, 5, 3, None, 0, entry=entry)                        # plain would take kernel 4 here
        assert (rc, c.kernel, c.nl) == (OK, 6, 1)
    # the 24-bit offsets of the LDS-DMA pieces: (ps * pitch + ch) * frames < 2^24 for y (75 frames) and for x in memory
    y_most = (1 << 24) // (75 * 11)
    assert nn(UV, 52, 75, 11, 4, .5, 0, entry="prepared", y_pitch=y_most - 1)[0] == OK
    assert nn(UV, 52, 75, 11, 4, .5, 0, entry="prepared", y_pitch=y_most + 1)[0] == EUNSUPPORTED
    x_most = (1 << 24) // (60 * 11)
    assert nn(UV, 52, 75, 11, 4, .5, 0, entry="grams", x_frames=60, x_pitch=x_most - 1)[0] == OK
    assert nn(UV, 52, 75, 11, 4, .5, 0, entry="grams", x_frames=60, x_pitch=x_most + 1)[0] == EUNSUPPORTED


def fold(UV, *a, fused=False, **kw):
    rc, c = UV.fold_choice(desc_of(*a, **kw), fused)
    return rc, (c.staged, c.shape, c.fw, c.fh, c.threads, c.nb)


def test_fold_choice(UV):
    at720 = dict(H=H720, W=W720)
    for fused in (False, True):
        assert fold(UV, 52, 75, 11, 4, 0.0, 0, fused=fused, **at720) == (OK, (1, 0, 64, 2, 512, 3))      # the ref view: 3 x 3 covering locations
        assert fold(UV, 52, 75, 3, 2, None, 0, fused=fused, **at720) == (OK, (1, 0, 64, 2, 512, 2))
        assert fold(UV, 52, 75, 5, 1, None, 0, fused=fused, H=720, W=1280)[1][5] == 0                    # 5 x 5: dynamic loops
        assert fold(UV, 52, 75, 11, 4, 0.0, 0x200, fused=fused, **at720)[1][5] == 0                      # bit 9
        assert fold(UV, 52, 75, 11, 4, 0.0, 0, fused=fused, pt=2, st=2, **at720)[1][5] == 0              # not the patch-major form
        assert fold(UV, 52, 75, 11, 4, 0.0, 2 << 12, fused=fused, **at720)[1][:5] == (1, 1, 32, 4, 512)  # bits 12-15: shape index + 1 ...
        free = fold(UV, 52, 500, 11, 4, 0.0, 0, fused=fused, **at720)
        assert free[1][0] == 1 and free[1][1] >= 3                                                       # (a 500-frame column: one-row tiles)
        assert fold(UV, 52, 500, 11, 4, 0.0, 1 << 12, fused=fused, **at720) == free                      # ... only when that shape fits
        assert fold(UV, 52, 75, 11, 4, 0.0, 9 << 12, fused=fused, **at720)[1][1] == 0                    # ... and exists
    assert fold(UV, 52, 75, 11, 4, 0.0, 1, **at720) == (OK, (0, -1, 0, 0, 256, 0))                       # vl3d_vote_fold, variant 1: unstaged
    assert fold(UV, 52, 75, 11, 4, 0.0, 1, fused=True, **at720)[1][0] == 1                               # the fused entry has the staged kernel only
    assert fold(UV, 5, 1300, 3, 2, None, 0)[1][0] == 0 and fold(UV, 5, 1300, 3, 2, None, 0, fused=True)[0] == EUNSUPPORTED      # no shape fits
    assert fold(UV, 65538, 75, 3, 2, None, 0)[0] == EINVAL
    rc, c = UV.fold_choice(desc_of(52, 75, 11, 4, 0.0, 0, **at720))
    assert c.lds_bytes == ((75 + 3) * 64 * 2 + (3 * 18 + 1) * 50) * 4 <= 53 * KIB                        # three workgroups per CU


def test_sweep_of_invariants(UV):
    from videoloop3d_amd import _lib as L
    f, out, seen = L.lib().vl3d_patchnn_choice, L.NNChoice(), set()
    ref = L.C.byref(out)
    rows6 = {(5, 4), (8, 2), (12, 1)}
    for tx, ty, ps, s, (pt, st), alpha in itertools.product(list(range(3, 131, 7)) + [200], list(range(3, 201, 11)) + [300], (3, 5, 7, 11), (1, 2, 4),
                                                            ((3, 1), (2, 2)), (None, 0.5)):
        d = desc_of(tx, ty, ps, s, alpha, 0, pt=pt, st=st)
        txu = (tx - pt) // st * st + pt
        tiles = -(-txu // 4) * -(-ty // 4)
        for low, bit11, entry in itertools.product(range(16), (0, 0x800), (0, 1, 2)):
            d.variant = low | bit11
            rc = f(d, entry, 1, d.W, tx, d.W, ref)
            assert rc in (OK, EINVAL, EUNSUPPORTED)
            if rc != OK:
                assert out.kernel == 0
                continue
            assert 0 < out.lds_bytes <= 150 * KIB and out.kernel in (2, 4, 6)
            if out.kernel == 6:
                assert 16 * out.nw >= txu and 16 * out.tyt >= ty and (out.tyt, out.nl) in rows6 and out.nw in (4, 8) and out.threads == 64 * out.nw
                assert out.xs == 16 or (out.xs == 14 and alpha is None and (pt, st) == (3, 1) and not bit11)
                assert out.ch >= 1 and out.scratch_layout == 1
            else:
                assert entry == 0 and out.scratch_layout == 2      # prepared inputs never name kernel 2 or 4
                if out.kernel == 4:
                    assert out.threads >= tiles and out.threads in (256, 512, 1024) and (not out.runsum or out.threads < 1024)
            seen.add(PR.instantiation(out))
    assert seen == PR.LAUNCH_TABLE      # nothing in the tables is unreachable, nothing is chosen outside them


def test_scratch_bytes_are_what_they_were(UV):
    """vl3d_patchnn_scratch_bytes is ABI (callers allocate by it): computed from the shared patch grid it returns the values recorded from the
    library of the commit before (tests/golden/make_patchnn_scratch_bytes.py is the recipe and the sweep)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_patchnn_scratch_bytes", os.path.join(ROOT, "tests", "golden", "make_patchnn_scratch_bytes.py"))
    recipe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recipe)
    ref = np.load(os.path.join(ROOT, "tests", "golden", "patchnn_scratch_bytes.npz"))
    assert list(ref["frames"]) == recipe.FRAMES and ref["sizes"].tolist() == [list(s) for s in recipe.SIZES] and ref["temporal"].tolist() == [list(t) for t in recipe.TEMPORAL]
    got = recipe.sweep(UV.L.lib().vl3d_patchnn_scratch_bytes)
    assert got.min() > 0 and np.array_equal(got, ref["bytes"])


def test_the_chooser_stands_alone_under_the_host_sanitizers(tmp_path):
    """the header compiles with plain g++ -std=c++17 (no HIP), and the stand-alone program of the named cases runs clean under
    -fsanitize=address,undefined"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the build environment"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "videoloop3d_amd", "csrc")]
    exe = str(tmp_path / "patchnn_choice_cases")
    # (the sanitizers' runtimes linked statically: the program does not depend on the order of the process's shared libraries)
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + inc + [os.path.join(ROOT, "tests", "patchnn_choice_cases.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failed" in p.stdout


def test_the_gpu_loss_tests_reach_every_instantiation(UV):
    """the shapes tests/test_gpu_loss.py searches at (tests/patchnn_rows.py) launch every row of the launch tables between them; the rows of
    NEW_CASES are the ones no other row reaches"""
    def reached(rows):
        got = set()
        for row in rows:
            rc, c = UV.patchnn_choice(PR.loss_desc(row))
            assert rc == OK, row
            got.add(PR.instantiation(c))
        return got
    assert reached(PR.ALL_ROWS) == PR.LAUNCH_TABLE
    new = [inst for _, inst in PR.NEW_CASES]
    assert [PR.instantiation(UV.patchnn_choice(PR.loss_desc(r))[1]) for r in PR.NEW_ROWS] == new
    assert reached(PR.TILE_COUNT_ROWS + PR.VARIANT_ROWS + PR.CLIP_LENGTH_ROWS + PR.ORACLE_ROWS) == PR.LAUNCH_TABLE - set(new)
