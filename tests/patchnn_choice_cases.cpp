// The named cases of the patch-NN search's and the vote-fold's choice (videoloop3d_amd/csrc/vl3d_patchnn_choice.h), run on the host with no GPU
// library:
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ivideoloop3d_amd/csrc tests/patchnn_choice_cases.cpp -o cases && ./cases
// tests/test_patchnn_choice_cpu.py builds and runs it; the same cases go through the exported vl3d_patchnn_choice() there.
#include <stdio.h>
#include "vl3d_patchnn_choice.h"

using namespace vl3d_loss_detail;

struct Call {
    int Tx, Ty, ps, stride;
    double alpha;                              // < 0: no alpha
    int variant, entry;
    bool has_scratch;
    // expected
    int status, kernel, a, b, c, d, ch, lds;   // kernel 6: a b c d = tyt nl nw xs; kernel 4: a b = runsum threads
};

static const int P = VL3D_NN_ENTRY_PLAIN, Y = VL3D_NN_ENTRY_PREPARED, G = VL3D_NN_ENTRY_GRAMS;
static const int OK = VL3D_OK, INV = VL3D_EINVAL, UNS = VL3D_EUNSUPPORTED;

// H, W = ps + 5 stride, ps + 9 stride (6 x 10 patch locations); pt 3, stridet 1
static const Call CALLS[] = {
    // Tx   Ty  ps  s  alpha  variant entry scratch  status kernel  instantiation  ch  lds
    {50,  75,  11, 4, .5,  6,     P, true,  OK,  6, 5,  4, 4, 16, 1, 45104},
    {12,  100, 5,  2, .5,  6,     P, true,  OK,  6, 8,  2, 4, 16, 3, 55232},
    {62,  128, 7,  3, -1., 6,     P, true,  OK,  6, 8,  2, 8, 14, 1, 76928},
    {82,  75,  5,  2, .5,  6,     P, true,  OK,  6, 5,  4, 8, 16, 2, 52368},
    {82,  122, 11, 4, .5,  6,     P, true,  OK,  6, 8,  2, 8, 16, 1, 73952},
    {122, 182, 7,  4, -1., 6,     P, true,  OK,  6, 12, 1, 8, 16, 1, 94672},
    {126, 190, 3,  2, .5,  6,     P, true,  OK,  6, 12, 1, 8, 16, 1, 101840},
    {30,  192, 5,  3, -1., 6,     P, true,  OK,  6, 12, 1, 4, 14, 1, 56640},
    {30,  192, 5,  3, -1., 0,     P, true,  OK,  4, 0,  512,  0, 0, 0, 37632},
    {82,  150, 11, 4, .5,  0,     P, true,  OK,  4, 0,  1024, 0, 0, 0, 65136},
    {30,  192, 11, 4, .5,  0,     P, true,  OK,  4, 1,  512,  0, 0, 0, 61824},
    {130, 200, 5,  2, -1., 0,     P, true,  OK,  2, 0,  0, 0, 0,  0, 148888},
    {50,  75,  5,  2, -1., 1,     P, true,  OK,  2, 0,  0, 0, 0,  0, 48868},
    {130, 75,  5,  2, -1., 6,     P, true,  INV, 0, 0,  0, 0, 0,  0, 0},
    {150, 260, 5,  2, -1., 0,     P, true,  INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 3,     P, true,  INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 0,     P, false, INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 6,     P, false, INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 0,     Y, false, INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 4,     Y, true,  INV, 0, 0,  0, 0, 0,  0, 0},
    {50,  75,  5,  2, -1., 4,     G, false, INV, 0, 0,  0, 0, 0,  0, 0},
    {130, 75,  5,  2, -1., 0,     Y, true,  UNS, 0, 0,  0, 0, 0,  0, 0},
    {50,  200, 5,  2, -1., 0,     G, false, UNS, 0, 0,  0, 0, 0,  0, 0},
    {58,  75,  5,  2, -1., 0,     P, true,  OK,  6, 5,  4, 4, 14, 2, 43664},
    {59,  75,  5,  2, -1., 0,     P, true,  OK,  6, 5,  4, 8, 14, 2, 48256},
    {59,  75,  5,  2, .5,  0,     P, true,  OK,  6, 5,  4, 4, 16, 2, 43984},
    {50,  75,  5,  2, -1., 0x806, P, true,  OK,  6, 5,  4, 4, 16, 2, 41104},
    {50,  75,  5,  2, -1., 0,     G, false, OK,  6, 5,  4, 4, 14, 2, 41104},
};

static vl3d_loss_desc desc_of(int Tx, int Ty, int H, int W, int ps, int stride, double alpha, int variant) {
    vl3d_loss_desc d{};
    d.Tx = Tx; d.Ty = Ty; d.H = H; d.W = W; d.ps = ps; d.pt = 3; d.stride = stride; d.stridet = 1;
    d.use_alpha = alpha >= 0; d.alpha = alpha >= 0 ? (float)alpha : 0.f;
    d.variant = variant;
    return d;
}

int main() {
    int bad = 0, n = 0;
    for (const Call &k : CALLS) {
        const vl3d_loss_desc d = desc_of(k.Tx, k.Ty, k.ps + 5 * k.stride, k.ps + 9 * k.stride, k.ps, k.stride, k.alpha, k.variant);
        const PatchNNChoice c = choose_patchnn(PatchNNFacts{&d, k.entry, k.has_scratch, d.W, d.Tx, d.W});
        bool ok = c.status == k.status && c.kernel == k.kernel && c.lds_bytes == k.lds && (c.status == OK) == (c.msg == nullptr);
        if (ok && c.kernel == 6) ok = c.tyt == k.a && c.nl == k.b && c.nw == k.c && c.xs == k.d && c.ch == k.ch && c.scratch_layout == VL3D_NN_LAYOUT_GRAM16;
        if (ok && c.kernel == 4) ok = c.runsum == k.a && c.threads == k.b && c.scratch_layout == VL3D_NN_LAYOUT_PIXEL_MAJOR;
        ++n;
        if (!ok) {
            ++bad;
            printf("FAIL (%d, %d, %d, %d, %g, 0x%x) entry %d scratch %d: status %d kernel %d tyt %d nl %d nw %d xs %d ch %d runsum %d threads %d lds %d\n", k.Tx,
                   k.Ty, k.ps, k.stride, k.alpha, k.variant, k.entry, k.has_scratch, c.status, c.kernel, c.tyt, c.nl, c.nw, c.xs, c.ch, c.runsum, c.threads, c.lds_bytes);
        }
    }
    // the fold at the 720p frame, 75 captured frames: {staged, shape, nb}; status for the fused entry when nothing fits
    struct Fold { int Tx, Ty, ps, stride, variant; bool fused; int status, staged, shape, nb; };
    static const Fold FOLDS[] = {
        {52, 75, 11, 4, 0, true, OK, 1, 0, 3},       {52, 75, 3, 2, 0, true, OK, 1, 0, 2},           {52, 75, 5, 1, 0, true, OK, 1, 4, 0},
        {52, 75, 11, 4, 0x200, true, OK, 1, 0, 0},   {52, 75, 11, 4, 2 << 12, false, OK, 1, 1, 3},   {52, 75, 11, 4, 1, false, OK, 0, -1, 0},
        {52, 75, 11, 4, 1, true, OK, 1, 0, 3},       {5, 1300, 3, 2, 0, false, OK, 0, -1, 0},        {5, 1300, 3, 2, 0, true, UNS, 0, 0, 0},
        {65538, 75, 3, 2, 0, false, INV, 0, 0, 0},
    };
    for (const Fold &k : FOLDS) {
        const int H = (720 - k.ps) / k.stride * k.stride + k.ps, W = (1280 - k.ps) / k.stride * k.stride + k.ps;
        const vl3d_loss_desc d = desc_of(k.Tx, k.Ty, H, W, k.ps, k.stride, -1., k.variant);
        const FoldChoice c = choose_fold(&d, k.fused);
        ++n;
        if (c.status != k.status || c.staged != k.staged || c.shape != k.shape || c.nb != k.nb || (c.staged && c.lds_bytes > LDS_MAX) ||
            (c.staged && (c.fw != fold_shapes[c.shape].fw || c.fh != fold_shapes[c.shape].fh || c.threads != fold_shapes[c.shape].nt))) {
            ++bad;
            printf("FAIL fold (%d, %d, %d, %d, 0x%x, fused %d): status %d staged %d shape %d nb %d lds %d\n", k.Tx, k.Ty, k.ps, k.stride, k.variant, k.fused,
                   c.status, c.staged, c.shape, c.nb, c.lds_bytes);
        }
    }
    // the scratch holds both layouts of every clip the search takes
    for (int Tx = 3; Tx <= 200; Tx += 7)
        for (int Ty = 3; Ty <= 200; Ty += 5) {
            const vl3d_loss_desc d = desc_of(Tx, Ty, 13, 21, 3, 2, -1., 0);
            const PatchGrid g = patch_grid_of(&d);
            const int64_t px = (int64_t)d.H * d.W;
            if (patchnn_scratch_bytes(&d) < px * 16 * (g.TxU + Ty) || patchnn_scratch_bytes(&d) < px * 12 * (g.TxP + g.TyP)) { ++bad; printf("FAIL scratch (%d, %d)\n", Tx, Ty); }
        }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
