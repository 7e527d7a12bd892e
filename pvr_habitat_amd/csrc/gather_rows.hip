// pvr_op_gather_rows (include/pvr_train.h): dst[i, :] = src[rows[i], :] - the one launch a prefix_cache pass adds: the boundary tensors of a pass's
// frames leave the dataset-sized cache for the staging buffer the trained ops read.  HBM-bound: n rows of 0.2 .. 3.2 MB are read once and written once.
// A row is cut into pieces of at most PIECE 16-byte lanes and the (row, piece) items are walked by a bounded grid, so that 2 rows of 3.2 MB and 334
// rows of 0.2 MB both spread over every CU.  Every source offset is a 64-bit product: the cache passes 4 GiB.  An index outside the source is never
// dereferenced; its row is filled with quiet NaNs.
#include <algorithm>
#include "common.h"
#include "../../include/pvr_train.h"

namespace pvr {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;                  // 16-byte loads in flight per lane
constexpr long long GATHER_PIECE = (long long)GATHER_THREADS * GATHER_UNROLL;       // lanes of 16 bytes per piece: 16 KiB
constexpr long long GATHER_MAX_BLOCKS = 8192;     // 32 workgroups per CU; the items past it are walked

__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_kernel(const u32x4 *__restrict__ src, long long n_src_rows, long long row_lanes,
                                                                     const long long *__restrict__ rows, long long pieces_per_row, long long items,
                                                                     u32x4 *__restrict__ dst) {
    const unsigned qnan = 0x7fc00000u;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long i = item / pieces_per_row, piece = item - i * pieces_per_row;
        const long long r = rows[i];              // (workgroup-uniform)
        const long long lo = piece * GATHER_PIECE, len = min(GATHER_PIECE, row_lanes - lo);
        u32x4 *d = dst + i * row_lanes + lo;
        if (r < 0 || r >= n_src_rows) {           // never dereferenced: the row shows as NaN
            const u32x4 nan4 = {qnan, qnan, qnan, qnan};
            for (long long j = threadIdx.x; j < len; j += GATHER_THREADS) d[j] = nan4;
            continue;
        }
        const u32x4 *s = src + r * row_lanes + lo;
        if (len == GATHER_PIECE) {                // a full piece: every lane's loads are issued before its first store
            u32x4 v[GATHER_UNROLL];
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u) v[u] = s[threadIdx.x + u * GATHER_THREADS];
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; ++u) d[threadIdx.x + u * GATHER_THREADS] = v[u];
        } else
            for (long long j = threadIdx.x; j < len; j += GATHER_THREADS) d[j] = s[j];
    }
}

}  // namespace pvr

extern "C" pvr_status pvr_op_gather_rows(const float *src, int64_t n_src_rows, int64_t row_floats, const int64_t *rows, int64_t n, float *dst,
                                         void *stream) {
    using namespace pvr;
    PVR_REQUIRE(src && rows && dst, "pvr_op_gather_rows: null argument");
    PVR_REQUIRE(n >= 1, "pvr_op_gather_rows: n = %lld rows to gather (at least 1)", (long long)n);
    PVR_REQUIRE(n_src_rows >= 1, "pvr_op_gather_rows: n_src_rows = %lld (the source holds at least one row)", (long long)n_src_rows);
    PVR_REQUIRE(row_floats >= 4 && row_floats % 4 == 0, "pvr_op_gather_rows: row_floats %lld must be a positive multiple of 4 (the lanes move 16 bytes)",
                (long long)row_floats);
    PVR_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "pvr_op_gather_rows: src_dev %p and dst_dev %p must be 16-byte aligned (the lanes "
                "move 16 bytes)", (const void *)src, (void *)dst);
    PVR_REQUIRE(((uintptr_t)rows & 7) == 0, "pvr_op_gather_rows: rows_dev %p is not 8-byte aligned (int64 indices)", (const void *)rows);
    const long long row_lanes = row_floats / 4;
    PVR_REQUIRE(row_lanes <= (1ll << 58) / n_src_rows && row_lanes <= (1ll << 58) / n, "pvr_op_gather_rows: %lld or %lld rows of %lld floats overflow a "
                "64-bit byte offset", (long long)n_src_rows, (long long)n, (long long)row_floats);
    const long long pieces = (row_lanes + GATHER_PIECE - 1) / GATHER_PIECE;
    const long long items = n * pieces;           // (n * row_lanes < 2^58: no overflow)
    const unsigned blocks = (unsigned)std::min(items, GATHER_MAX_BLOCKS);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream, (const u32x4 *)src, (long long)n_src_rows, row_lanes,
                       (const long long *)rows, pieces, items, (u32x4 *)dst);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}
