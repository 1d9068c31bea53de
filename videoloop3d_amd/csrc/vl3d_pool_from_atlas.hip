// A viewer package's atlases -> the baked pool (include/vl3d.h "A viewer package's atlases"; videoloop3d_amd/baked.py: open_viewer_package).
//
// The package stores the RGBA8 tiles of the kept quads in two atlases, row-major grids of th x tw-texel tiles: static tiles once, dynamic
// tiles per frame.  vl3d_render_fwd_baked_pool reads the same texels as 8 x 8 blocks (256 bytes) behind the block table of
// packed.PackedLayout in the tile-exact layout (a plane is QH x QW tiles of th x tw texels).  This unit moves one frame of tiles into those
// blocks:
//   * one wave per block of the table, one lane per texel: the table entry is wave-uniform (a block without storage, and a static block in a
//     frame other than 0, return before any other load), the store is the block's 256 contiguous bytes as 64 dwords;
//   * per lane one tile_src entry (shared by the lanes of a tile) and one dword of its atlas; a texel past the plane is 0 (what pack_() and
//     bake_pool leave there), a texel of a culled tile is `culled`;
//   * a static tile inside a dynamic block is written in every frame (the block owns T slots).
// No LDS, no scratch.
#include "vl3d_common.h"

namespace {

constexpr int TSB = 8;      // block side (vl3d_adam_window_tile())

struct AtlasSrc {
    const unsigned *texels;      // [h][w] RGBA8 words, or nullptr when n_tiles == 0
    int w, gw, n_tiles;          // width in texels, tiles per row, tiles in the grid
};

struct FromAtlasArgs {
    int n_blocks, tiles_y, tiles_x;      // blocks of the table: D * tiles_y * tiles_x
    int Hs, Ws, th, tw, QH, QW, frame;
    const int *blocks, *tile_src;
    AtlasSrc atlas[2];                   // [0] static, [1] dynamic (the frame this call carries)
    unsigned culled;
    unsigned *pool;
};

__global__ __launch_bounds__(256) void pool_from_atlas_k(FromAtlasArgs a) {
    const int blk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (blk >= a.n_blocks) return;
    const int e = __builtin_amdgcn_readfirstlane(a.blocks[blk]);
    if (e < 0) return;                                // not stored: nothing else is loaded
    if (!(e & 1) && a.frame != 0) return;             // a static block is written once, with frame 0
    const int lane = threadIdx.x & 63;
    const int bx = blk % a.tiles_x, rest = blk / a.tiles_x;
    const int by = rest % a.tiles_y, d = rest / a.tiles_y;
    const int y = by * TSB + (lane >> 3), x = bx * TSB + (lane & 7);
    unsigned w = 0u;                                  // past the plane's last row / column
    if (y < a.Hs && x < a.Ws) {
        const int qy = y / a.th, qx = x / a.tw;       // < QH, QW: Hs = QH th, Ws = QW tw (checked by the entry)
        const int src = a.tile_src[((size_t)d * a.QH + qy) * a.QW + qx];
        w = a.culled;
        if (src >= 0) {
            const AtlasSrc &s = a.atlas[src & 1];
            const int k = src >> 1;
            if (k < s.n_tiles) {                      // n_tiles = (h / th) * (w / tw): every texel of tile k lies inside the atlas
                const int row = (k / s.gw) * a.th + (y - qy * a.th), col = (k % s.gw) * a.tw + (x - qx * a.tw);
                w = s.texels[(size_t)row * s.w + col];
            }
        }
    }
    a.pool[((size_t)(e >> 1) + ((e & 1) ? a.frame : 0)) * (TSB * TSB) + lane] = w;
}

}  // namespace

extern "C" int vl3d_pool_from_atlas_rgba8(int32_t D, int32_t T, int32_t Hs, int32_t Ws, int32_t th, int32_t tw, int32_t QH, int32_t QW,
                                          const int32_t *blocks, const int32_t *tile_src, const uint8_t *static_atlas, int32_t As_h, int32_t As_w,
                                          const uint8_t *dyn_atlas, int32_t Ad_h, int32_t Ad_w, int32_t frame, uint32_t culled_rgba8,
                                          uint8_t *pool, vl3d_stream_t stream) {
    VL3D_REQUIRE(D > 0 && T > 0 && th > 0 && tw > 0 && QH > 0 && QW > 0, "vl3d_pool_from_atlas_rgba8: D, T, th, tw, QH, QW >= 1");
    VL3D_REQUIRE((int64_t)QH * th == Hs && (int64_t)QW * tw == Ws,
                 "vl3d_pool_from_atlas_rgba8: the destination is the tile-exact layout of the quad maps (Hs = QH th, Ws = QW tw)");
    VL3D_REQUIRE(frame >= 0 && frame < T, "vl3d_pool_from_atlas_rgba8: frame outside [0, T)");
    VL3D_REQUIRE(blocks && tile_src && pool, "vl3d_pool_from_atlas_rgba8: null pointer");
    VL3D_REQUIRE(As_h >= 0 && As_w >= 0 && Ad_h >= 0 && Ad_w >= 0 && (As_h == 0) == (As_w == 0) && (Ad_h == 0) == (Ad_w == 0),
                 "vl3d_pool_from_atlas_rgba8: an atlas is As_h x As_w texels, or 0 x 0 when the package has no such tiles");
    VL3D_REQUIRE((static_atlas != nullptr) == (As_h > 0) && (dyn_atlas != nullptr) == (Ad_h > 0),
                 "vl3d_pool_from_atlas_rgba8: an atlas pointer is NULL exactly when its size is 0 x 0");
    VL3D_REQUIRE(((uintptr_t)static_atlas & 3) == 0 && ((uintptr_t)dyn_atlas & 3) == 0 && ((uintptr_t)pool & 3) == 0 &&
                 ((uintptr_t)blocks & 3) == 0 && ((uintptr_t)tile_src & 3) == 0,
                 "vl3d_pool_from_atlas_rgba8: the atlases, the pool, the block table and tile_src must be 4-byte aligned");
    VL3D_REQUIRE(As_h % th == 0 && As_w % tw == 0 && Ad_h % th == 0 && Ad_w % tw == 0,
                 "vl3d_pool_from_atlas_rgba8: the atlas sizes must be multiples of the tile size");
    const int tiles_y = (Hs + TSB - 1) / TSB, tiles_x = (Ws + TSB - 1) / TSB;
    const int64_t n_blocks = (int64_t)D * tiles_y * tiles_x;
    VL3D_REQUIRE(n_blocks <= INT32_MAX - 4 && (int64_t)(As_h / th) * (As_w / tw) <= INT32_MAX / 2 && (int64_t)(Ad_h / th) * (Ad_w / tw) <= INT32_MAX / 2,
                 "vl3d_pool_from_atlas_rgba8: block table or atlas grid too large for 31-bit indices");
    FromAtlasArgs a;
    a.n_blocks = (int)n_blocks; a.tiles_y = tiles_y; a.tiles_x = tiles_x;
    a.Hs = Hs; a.Ws = Ws; a.th = th; a.tw = tw; a.QH = QH; a.QW = QW; a.frame = frame;
    a.blocks = blocks; a.tile_src = tile_src;
    a.atlas[0] = AtlasSrc{reinterpret_cast<const unsigned *>(static_atlas), As_w, As_w / tw, (As_h / th) * (As_w / tw)};
    a.atlas[1] = AtlasSrc{reinterpret_cast<const unsigned *>(dyn_atlas), Ad_w, Ad_w / tw, (Ad_h / th) * (Ad_w / tw)};
    a.culled = culled_rgba8;
    a.pool = reinterpret_cast<unsigned *>(pool);
    hipLaunchKernelGGL(pool_from_atlas_k, dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
