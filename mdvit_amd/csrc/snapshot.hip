// A set of separate tensors <-> one flat buffer in ONE launch (mdvit_amd/snapshot.py: the `torch.save(model.state_dict(), best_model_dir)` of
// multi_train_MDViT.py's train loop is one device-to-host copy and one synchronisation per tensor, 608 to 1460 of them).
// A device table of {tensor pointer, byte offset in the flat buffer, nbytes} rows drives the kernel (grid.y = table row), one row per chunk of a
// tensor, as the optimizer's table is chunked (csrc/optim.hip).  The copy is byte-exact and dtype-blind: a state_dict holds int64 counters next to
// the fp32 weights, and a tensor may be a view that is only 4-byte aligned, so each row picks its own access width.
#include "common.h"

namespace {

// PACK: tensor -> flat[offset ..];  !PACK: flat[offset ..] -> tensor.  Bytes outside [0, nbytes) of either side are never touched.
template <bool PACK>
__global__ __launch_bounds__(256) void table_copy_kernel(const long long* __restrict__ table, unsigned char* flat) {
    const long long* row = table + 3 * (long)blockIdx.y;
    unsigned char* t = reinterpret_cast<unsigned char*>(row[0]);
    unsigned char* f = flat + row[1];
    const long n = (long)row[2];
    const unsigned char* src = PACK ? t : f;
    unsigned char* dst = PACK ? f : t;
    const uintptr_t both = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst);
    const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long done = 0;
    if ((both & 15) == 0) {
        const long nq = n >> 4;
        for (long q = t0; q < nq; q += stride) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(src)[q];
        done = nq << 4;
    } else if ((both & 3) == 0) {
        const long nw = n >> 2;
        for (long w = t0; w < nw; w += stride) reinterpret_cast<uint32_t*>(dst)[w] = reinterpret_cast<const uint32_t*>(src)[w];
        done = nw << 2;
    }
    for (long i = done + t0; i < n; i += stride) dst[i] = src[i];          // the byte tail (all of the row if a side is not even 4-byte aligned)
}

template <bool PACK>
int table_copy(const void* table_dev, int32_t n_rows, unsigned char* flat, int32_t blocks_per_row, hipStream_t s) {
    // gridDim.y is limited to 65535: a longer table goes out in slices, as mdvit_adamw_step slices its table
    for (int32_t r0 = 0; r0 < n_rows; r0 += 65535) {
        const int32_t nr = n_rows - r0 < 65535 ? n_rows - r0 : 65535;
        hipLaunchKernelGGL(table_copy_kernel<PACK>, dim3(blocks_per_row, nr), dim3(256), 0, s, (const long long*)table_dev + 3 * (long long)r0, flat);
        MDVIT_LAUNCH_CHECK();
    }
    return MDVIT_OK;
}

}  // namespace

extern "C" int mdvit_table_pack(const void* table_dev, int32_t n_rows, void* dst, int32_t blocks_per_row, void* stream) {
    MDVIT_CHECK_ARG(table_dev && dst, MDVIT_E_SHAPE, "table_pack: null table or destination");
    MDVIT_CHECK_ARG(n_rows > 0 && blocks_per_row > 0 && blocks_per_row <= 65535, MDVIT_E_SHAPE, "table_pack: n_rows %d / blocks_per_row %d out of range", (int)n_rows, (int)blocks_per_row);
    MDVIT_CHECK_ARG(aligned16(dst), MDVIT_E_ALIGN, "table_pack: the flat buffer must be 16-byte aligned");
    return table_copy<true>(table_dev, n_rows, (unsigned char*)dst, blocks_per_row, (hipStream_t)stream);
}

extern "C" int mdvit_table_unpack(const void* table_dev, int32_t n_rows, const void* src, int32_t blocks_per_row, void* stream) {
    MDVIT_CHECK_ARG(table_dev && src, MDVIT_E_SHAPE, "table_unpack: null table or source");
    MDVIT_CHECK_ARG(n_rows > 0 && blocks_per_row > 0 && blocks_per_row <= 65535, MDVIT_E_SHAPE, "table_unpack: n_rows %d / blocks_per_row %d out of range", (int)n_rows, (int)blocks_per_row);
    MDVIT_CHECK_ARG(aligned16(src), MDVIT_E_ALIGN, "table_unpack: the flat buffer must be 16-byte aligned");
    return table_copy<false>(table_dev, n_rows, (unsigned char*)const_cast<void*>(src), blocks_per_row, (hipStream_t)stream);
}
