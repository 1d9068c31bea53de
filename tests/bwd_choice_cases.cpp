// The named cases of the render backward's choice (videoloop3d_amd/csrc/vl3d_render_bwd_choice.h), run on the host with no GPU library:
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ivideoloop3d_amd/csrc tests/bwd_choice_cases.cpp -o cases && ./cases
// tests/test_bwd_choice_cpu.py builds and runs it; the same cases go through the exported vl3d_render_bwd_choice() there.
#include <stdio.h>
#include "vl3d_render_bwd_choice.h"

using namespace vl3d_render_detail;

struct Call {
    const char *name;
    int entry, variant, T;
    double stack_scale;                        // the stack's size over the 720p frame's
    bool reg, qk, gcu, f16, tile_ok;
    int coord, ract;
    // expected
    int family, width, rows;
    bool x_reg, x_mask, x_adam, x_cull, x_owner4, x_gather9;
};

static const int R = VL3D_BWD_ENTRY_RENDER, M = VL3D_BWD_ENTRY_MASK, A = VL3D_BWD_ENTRY_ADAM;
static const int AFF = VL3D_COORD_AFFINE, UTL = VL3D_COORD_UTILS_MPI, SIG = VL3D_ACT_SIGMOID;
static const int ATOM = VL3D_BWD_ATOMICS, TILE = VL3D_BWD_TILE, PAIR = VL3D_BWD_PAIR, P12 = VL3D_BWD_PAIR12;

static const Call CALLS[] = {
    //                                   entry v  T  scale reg    qk     gcu    f16    ok     coord ract           family w  rows reg    mask   adam   cull   own4   g9
    {"cfg3 variant 0",                   R, 0, 50, 1.0, false, false, false, false, true,  AFF, SIG,            P12,  64, 12, false, false, false, false, false, false},
    {"cfg3 variant 6",                   R, 6, 50, 1.0, false, false, false, false, true,  AFF, SIG,            PAIR, 32, 16, false, false, false, false, false, false},
    {"cfg3 variant 7",                   R, 7, 50, 1.0, false, false, false, false, true,  AFF, SIG,            P12,  64, 12, false, false, false, false, false, false},
    {"cfg3 variant 3",                   R, 3, 50, 1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 16, false, false, false, false, false, false},
    {"cfg3 variant 4",                   R, 4, 50, 1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 16, false, false, false, false, false, true},
    {"cfg3 variant 1",                   R, 1, 50, 1.0, false, false, false, false, true,  AFF, SIG,            ATOM, 0,  0,  false, false, false, false, false, false},
    {"cfg3 short scratch / uv noise",    R, 0, 50, 1.0, false, false, false, false, false, AFF, SIG,            ATOM, 0,  0,  false, false, false, false, false, false},
    {"1.1x stack",                       R, 0, 50, 1.1, false, false, false, false, true,  AFF, SIG,            TILE, 64, 16, false, false, false, false, false, false},
    {"1.1x stack, regularisers",         R, 0, 50, 1.1, true,  false, false, false, true,  AFF, SIG,            PAIR, 32, 16, true,  false, false, false, false, false},
    {"1.1x, regularisers, utils_mpi",    R, 0, 50, 1.1, true,  false, false, false, true,  UTL, SIG,            TILE, 64, 16, true,  false, false, false, false, false},
    {"T = 1 variant 0",                  R, 0, 1,  1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 8,  false, false, false, false, true,  false},
    {"T = 1 variant 3",                  R, 3, 1,  1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 16, false, false, false, false, false, false},
    {"T = 1 fp16 stack",                 R, 0, 1,  1.0, false, false, false, true,  true,  AFF, SIG,            TILE, 64, 16, false, false, false, false, true,  false},
    {"quad map without gcu",             R, 0, 50, 1.0, false, true,  false, false, true,  AFF, SIG,            TILE, 64, 16, false, false, false, true,  false, false},
    {"quad map with gcu, variant 0",     R, 0, 50, 1.0, false, true,  true,  false, true,  AFF, SIG,            TILE, 32, 16, false, false, false, true,  false, false},
    {"quad map with gcu, variant 3",     R, 3, 50, 1.0, false, true,  true,  false, true,  AFF, SIG,            TILE, 64, 16, true,  false, false, true,  false, false},
    {"mask entry, default",              M, 0, 1,  1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 8,  false, true,  false, false, true,  false},
    {"mask entry, variant 3",            M, 3, 1,  1.0, false, false, false, false, true,  AFF, SIG,            TILE, 64, 16, false, true,  false, false, false, false},
    {"fused step, dense",                A, 0, 50, 1.0, false, false, false, false, true,  AFF, SIG,            PAIR, 32, 16, false, false, true,  false, false, false},
    {"fused step, culled",               A, 0, 50, 1.0, false, true,  true,  false, true,  AFF, SIG,            TILE, 32, 16, true,  false, true,  true,  false, false},
    {"fused step, culled, variant 3",    A, 3, 50, 1.0, false, true,  true,  false, true,  AFF, SIG,            TILE, 64, 16, true,  false, true,  true,  false, false},
    {"variant 6 with regularisers",      R, 6, 50, 1.0, true,  false, false, false, true,  AFF, SIG,            TILE, 64, 16, true,  false, false, false, false, false},
    {"variant 7 with regularisers",      R, 7, 50, 1.0, true,  false, false, false, true,  AFF, SIG,            TILE, 64, 16, true,  false, false, false, false, false},
    {"(none, sigmoid) activations",      R, 0, 50, 1.0, false, false, false, false, true,  AFF, VL3D_ACT_NONE,  TILE, 64, 16, false, false, false, false, false, false},
};

int main() {
    int bad = 0;
    for (const Call &k : CALLS) {
        BwdFacts f{};
        f.coord = k.coord; f.border = k.coord == AFF ? VL3D_BORDER_HARDCUT : VL3D_BORDER_ZEROS; f.order = k.coord == AFF ? VL3D_ACT_POST : VL3D_ACT_PRE;
        f.ract = k.ract; f.aact = SIG; f.f16 = k.f16; f.plane_record = 9;
        f.T = k.T; f.H = 720; f.W = 1280; f.Hs = (int)(720 * k.stack_scale); f.Ws = (int)(1280 * k.stack_scale);
        f.set = bwd_setting_of(k.entry, k.variant, k.tile_ok, k.qk);
        f.reg = k.reg; f.mask = k.entry == M; f.adam = k.entry == A; f.qk = k.qk; f.gcu = k.gcu;
        const BwdChoice c = choose_bwd(f);
        const bool none = c.family == ATOM;
        const bool ok = c.family == k.family && (none || (BWD_REGIONS[c.shape].width == k.width && BWD_REGIONS[c.shape].rows == k.rows)) &&
                        c.reg == k.x_reg && c.mask == k.x_mask && c.adam == k.x_adam && c.cull == k.x_cull && c.f16 == (k.f16 && !none) &&
                        c.owner4 == k.x_owner4 && f.set.gather9 == k.x_gather9;
        if (!ok) {
            ++bad;
            printf("FAIL %s: family %d, %d x %d, reg %d mask %d adam %d cull %d f16 %d owner4 %d gather9 %d\n", k.name, c.family, BWD_REGIONS[c.shape].width,
                   BWD_REGIONS[c.shape].rows, c.reg, c.mask, c.adam, c.cull, c.f16, c.owner4, f.set.gather9);
        }
    }
    // every shape's window records fit the count the scratch layout is sized by
    for (int H = 1; H <= 200; ++H)
        for (int W = 1; W <= 200; ++W)
            for (int s = 0; s < BWD_NSHAPES; ++s) {
                const int64_t n = (int64_t)((W + bwd_interior_w(s) - 1) / bwd_interior_w(s)) * ((H + bwd_interior_h(s) - 1) / bwd_interior_h(s));
                if (n > bwd_max_tiles(H, W)) { ++bad; printf("FAIL bwd_max_tiles(%d, %d) < shape %d's %lld\n", H, W, s, (long long)n); }
            }
    printf("%d cases, %d failed\n", (int)(sizeof CALLS / sizeof CALLS[0]), bad);
    return bad ? 1 : 0;
}
