// Trimming a baked pool (include/vl3d.h "Trimming a baked pool"; videoloop3d_amd/baked.py: BakedPool.trimmed).
//
// A one-off conversion over the RGBA8 blocks behind the block table of packed.PackedLayout: which texels can a player ever show, which of
// them change over the loop, and from that which blocks need no storage, which dynamic blocks are one static block stored T times.  Three
// kernels, each one wave per block of the table and one lane per texel (a block is 8 x 8 texels = 64 dwords = 256 contiguous bytes):
//   * trim_flags_k: per texel, over the block's frames, bit 0 "some frame has an alpha byte > 0", bit 1 "some frame's four bytes differ from
//     frame 0's" -> a (D, Hs, Ws) byte map.  T dword loads per lane of a dynamic block, 1 of a static one, none of a block without storage
//     (its texels are `culled`, a kernel argument);
//   * trim_class_k: per texel the 3 x 3 neighbourhood of that map (clipped to the plane) -> show = some neighbour has bit 0,
//     moves = show and the texel's own bit 1; both reduced over the wave with __ballot -> the block's new slot count 0 / 1 / T;
//   * trim_move_k: one wave per (block, frame): 256 bytes from the old slot to the new one, for the frames the new table keeps.
// The exclusive scan of the slot counts between the second and the third kernel is the caller's (torch.cumsum, as PackedLayout builds its
// table).  Memory bound; no LDS, no atomics, no scratch memory; every store has one writer, so the result is bit-for-bit deterministic.
#include "vl3d_common.h"

namespace {

constexpr int TSB = 8;      // block side (vl3d_adam_window_tile())

struct TrimArgs {
    int T, Hs, Ws, tiles_x, bpp;         // bpp: blocks per plane = ceil(Hs / 8) * ceil(Ws / 8)
    int64_t n_slots;                     // slots of `pool`
    const int *blocks;                   // [D][bpp]
    const unsigned *pool;                // [n_slots][64] RGBA8 words
    unsigned culled;
    uint8_t *flags;                      // [D][Hs][Ws]
    int *slots;                          // [D][bpp]: the new slot count
    uint8_t *texel_class;                // [D][Hs][Ws]
};

// the table entry of block (d, b) as the three kernels read it: an entry whose slots would leave the pool counts as not stored
__device__ __forceinline__ int trim_entry(const int *blocks, size_t i, int T, int64_t n_slots) {
    const int e = __builtin_amdgcn_readfirstlane(blocks[i]);
    if (e < 0) return -1;
    return ((int64_t)(e >> 1) + ((e & 1) ? T : 1) <= n_slots) ? e : -1;
}

__global__ __launch_bounds__(256) void trim_flags_k(TrimArgs a) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (b >= a.bpp) return;
    const int d = blockIdx.y, lane = threadIdx.x & 63;
    const int e = trim_entry(a.blocks, (size_t)d * a.bpp + b, a.T, a.n_slots);
    const int y = (b / a.tiles_x) * TSB + (lane >> 3), x = (b % a.tiles_x) * TSB + (lane & 7);
    unsigned vis = (a.culled >> 24) != 0u, dif = 0u;
    if (e >= 0) {                                          // (wave-uniform)
        const unsigned *src = a.pool + (size_t)(e >> 1) * (TSB * TSB) + lane;
        const unsigned w0 = src[0];
        vis = (w0 >> 24) != 0u;
        const int n = (e & 1) ? a.T : 1;
        for (int t = 1; t < n; ++t) {
            const unsigned w = src[(size_t)t * (TSB * TSB)];
            vis |= (w >> 24) != 0u;
            dif |= w != w0;
        }
    }
    if (y < a.Hs && x < a.Ws) a.flags[((size_t)d * a.Hs + y) * a.Ws + x] = (uint8_t)(vis | dif << 1);
}

__global__ __launch_bounds__(256) void trim_class_k(TrimArgs a) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (b >= a.bpp) return;
    const int d = blockIdx.y, lane = threadIdx.x & 63;
    const int e = trim_entry(a.blocks, (size_t)d * a.bpp + b, a.T, a.n_slots);
    const int y = (b / a.tiles_x) * TSB + (lane >> 3), x = (b % a.tiles_x) * TSB + (lane & 7);
    const bool inside = y < a.Hs && x < a.Ws;
    unsigned own = 0u, any = 0u;
    if (inside) {
        const uint8_t *plane = a.flags + (size_t)d * a.Hs * a.Ws;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= a.Hs || xx < 0 || xx >= a.Ws) continue;      // out of the plane counts as 0
                const unsigned f = plane[(size_t)yy * a.Ws + xx];
                if (dy == 0 && dx == 0) own = f;
                any |= f & 1u;
            }
        }
    }
    const bool show = inside && any != 0u, moves = show && (own & 2u) != 0u;
    if (inside) a.texel_class[((size_t)d * a.Hs + y) * a.Ws + x] = (uint8_t)((unsigned)show | (unsigned)moves << 1);
    const unsigned long long shows = __ballot(show), moving = __ballot(moves);
    int n = 0;
    if (e >= 0 && (shows != 0ull || (a.culled >> 24) != 0u)) n = ((e & 1) && moving != 0ull) ? a.T : 1;
    if (lane == 0) a.slots[(size_t)d * a.bpp + b] = n;
}

struct MoveArgs {
    int T, bpp;
    int64_t n_slots, new_n_slots;
    const int *blocks, *new_blocks;      // [D][bpp]
    const unsigned *pool;
    unsigned *new_pool;
};

__global__ __launch_bounds__(256) void trim_move_k(MoveArgs a) {
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));      // < bpp * T + 4 <= INT32_MAX (the entry)
    const int b = w / a.T, t = w % a.T;
    if (b >= a.bpp) return;
    const size_t i = (size_t)blockIdx.y * a.bpp + b;
    const int en = trim_entry(a.new_blocks, i, a.T, a.new_n_slots);
    if (en < 0 || t >= ((en & 1) ? a.T : 1)) return;
    const int eo = trim_entry(a.blocks, i, a.T, a.n_slots);
    if (eo < 0 || ((en & 1) && !(eo & 1))) return;         // a kept block was stored; a block never becomes dynamic
    const int lane = threadIdx.x & 63;
    a.new_pool[((size_t)(en >> 1) + t) * (TSB * TSB) + lane] = a.pool[((size_t)(eo >> 1) + t) * (TSB * TSB) + lane];
}

int trim_dims(int32_t D, int32_t T, int32_t Hs, int32_t Ws, int *tiles_x, int *bpp) {
    VL3D_REQUIRE(D >= 1 && T >= 1 && Hs >= 1 && Ws >= 1, "vl3d_baked_trim: D, T, Hs, Ws >= 1");
    VL3D_REQUIRE(D <= 65535, "vl3d_baked_trim: D <= 65535 (one grid row per plane)");
    const int64_t ty = ((int64_t)Hs + TSB - 1) / TSB, tx = ((int64_t)Ws + TSB - 1) / TSB;
    VL3D_REQUIRE(ty * tx * T <= INT32_MAX - 4, "vl3d_baked_trim: blocks per plane times T too large for 31-bit indices");
    *tiles_x = (int)tx;
    *bpp = (int)(ty * tx);
    return VL3D_OK;
}

}  // namespace

extern "C" int64_t vl3d_baked_trim_scratch_bytes(int32_t D, int32_t Hs, int32_t Ws) {
    if (D < 1 || Hs < 1 || Ws < 1) return 0;
    return ((int64_t)D * Hs * Ws + 255) / 256 * 256;
}

extern "C" int vl3d_baked_trim_classify(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const int32_t *blocks, const uint8_t *pool, int64_t n_slots,
                                        uint32_t culled_rgba8, void *scratch, int64_t scratch_bytes, int32_t *block_slots,
                                        uint8_t *texel_class, vl3d_stream_t stream) {
    int tiles_x, bpp;
    if (int rc = trim_dims(D, T, Hs, Ws, &tiles_x, &bpp)) return rc;
    VL3D_REQUIRE(blocks && scratch && block_slots && texel_class && n_slots >= 0 && (pool || n_slots == 0),
                 "vl3d_baked_trim_classify: null pointer (the pool may be NULL only with n_slots == 0)");
    VL3D_REQUIRE(((uintptr_t)blocks & 3) == 0 && ((uintptr_t)pool & 3) == 0 && ((uintptr_t)block_slots & 3) == 0,
                 "vl3d_baked_trim_classify: the block table, the pool and block_slots must be 4-byte aligned");
    VL3D_REQUIRE((void *)texel_class != scratch, "vl3d_baked_trim_classify: texel_class is another buffer than scratch");
    VL3D_REQUIRE(scratch_bytes >= vl3d_baked_trim_scratch_bytes(D, Hs, Ws),
                 "vl3d_baked_trim_classify: scratch smaller than vl3d_baked_trim_scratch_bytes(D, Hs, Ws)");
    TrimArgs a;
    a.T = T; a.Hs = Hs; a.Ws = Ws; a.tiles_x = tiles_x; a.bpp = bpp;
    a.n_slots = n_slots;
    a.blocks = blocks;
    a.pool = reinterpret_cast<const unsigned *>(pool);
    a.culled = culled_rgba8;
    a.flags = static_cast<uint8_t *>(scratch);
    a.slots = block_slots;
    a.texel_class = texel_class;
    const dim3 grid((unsigned)((bpp + 3) / 4), (unsigned)D);
    hipLaunchKernelGGL(trim_flags_k, grid, dim3(256), 0, (hipStream_t)stream, a);
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(trim_class_k, grid, dim3(256), 0, (hipStream_t)stream, a);      // (stream order: the flag map is complete)
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_baked_trim_move(int32_t D, int32_t T, int32_t Hs, int32_t Ws, const int32_t *blocks, const uint8_t *pool, int64_t n_slots,
                                    const int32_t *new_blocks, uint8_t *new_pool, int64_t new_n_slots, vl3d_stream_t stream) {
    int tiles_x, bpp;
    if (int rc = trim_dims(D, T, Hs, Ws, &tiles_x, &bpp)) return rc;
    VL3D_REQUIRE(blocks && new_blocks && n_slots >= 0 && new_n_slots >= 0 && (pool || n_slots == 0) && (new_pool || new_n_slots == 0),
                 "vl3d_baked_trim_move: null pointer (a pool may be NULL only with 0 slots)");
    VL3D_REQUIRE(((uintptr_t)blocks & 3) == 0 && ((uintptr_t)new_blocks & 3) == 0 && ((uintptr_t)pool & 3) == 0 && ((uintptr_t)new_pool & 3) == 0,
                 "vl3d_baked_trim_move: the block tables and the pools must be 4-byte aligned");
    VL3D_REQUIRE(pool != new_pool || n_slots == 0, "vl3d_baked_trim_move: the new pool is another buffer than the old one");
    if (new_n_slots == 0) return VL3D_OK;      // nothing is kept
    MoveArgs a;
    a.T = T; a.bpp = bpp;
    a.n_slots = n_slots; a.new_n_slots = new_n_slots;
    a.blocks = blocks; a.new_blocks = new_blocks;
    a.pool = reinterpret_cast<const unsigned *>(pool);
    a.new_pool = reinterpret_cast<unsigned *>(new_pool);
    hipLaunchKernelGGL(trim_move_k, dim3((unsigned)(((int64_t)bpp * T + 3) / 4), (unsigned)D), dim3(256), 0, (hipStream_t)stream, a);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
