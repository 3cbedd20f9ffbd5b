// nn_reduce.hip -- deterministic reductions of the SELD CRNN (C ABI: include/salsa_nn.h; internal: nn_det.h): the per-device
// workspace of the deterministic mode, the fixed-order sum of the weight gradients' per-workgroup slabs, and the column sums.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>

#include "../../include/salsa_nn.h"
#include "nn_det.h"

namespace {

// ------------------------------------------------------------------------------------------------ deterministic reductions
// dw[i] += sum over the slabs of ws[slab][i], in a FIXED order (what makes the result reproducible; it need not be slab order): a
// workgroup owns 4 * 256 / SL consecutive elements and its SL slab lanes each add every SL-th slab in ascending order, then the SL
// partial sums are added in lane order.  (First version: one thread per four elements walking all slabs -- 4 to 36
// workgroups for the first layer's 1280 slabs and the 64 -> 64 layers' 384: 138 / 33 us per call.)
template <int SL> // slab lanes per workgroup (16: many slabs -- the 64 -> 64 and first-layer gradients; 4: the wide layers' 4 - 64 slabs)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ ws, int slabs, long n, float *__restrict__ dw)
{
    constexpr int EX = 256 / SL;
    __shared__ float4 red[SL][EX];
    const int ex = threadIdx.x % EX, sl = threadIdx.x / EX;
    const long i = ((long)blockIdx.x * EX + ex) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i + 3 < n) {
        int s = sl;
        for (; s + 3 * SL < slabs; s += 4 * SL) { // four loads in flight; the additions keep their order
            const float4 a = *(const float4 *)(ws + (long)s * n + i), b = *(const float4 *)(ws + (long)(s + SL) * n + i);
            const float4 c = *(const float4 *)(ws + (long)(s + 2 * SL) * n + i), d = *(const float4 *)(ws + (long)(s + 3 * SL) * n + i);
            acc.x = (((acc.x + a.x) + b.x) + c.x) + d.x; acc.y = (((acc.y + a.y) + b.y) + c.y) + d.y;
            acc.z = (((acc.z + a.z) + b.z) + c.z) + d.z; acc.w = (((acc.w + a.w) + b.w) + c.w) + d.w;
        }
        for (; s < slabs; s += SL) {
            const float4 a = *(const float4 *)(ws + (long)s * n + i);
            acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
        }
    } else if (i < n) { // (n not a multiple of 4: the last elements one by one)
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s = sl; s < slabs; s += SL)
            for (int k = 0; k < 4 && i + k < n; k++) t[k] += ws[(long)s * n + i + k];
        acc = make_float4(t[0], t[1], t[2], t[3]);
    }
    red[sl][ex] = acc;
    __syncthreads();
    if (sl == 0 && i < n) {
        float4 t = red[0][ex];
#pragma unroll
        for (int k = 1; k < SL; k++) {
            const float4 v = red[k][ex];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const float o[4] = {t.x, t.y, t.z, t.w};
        for (int k = 0; k < 4 && i + k < n; k++) dw[i + k] += o[k];
    }
}

__global__ __launch_bounds__(256) void slab_reduce_strided_kernel(const float *__restrict__ ws, int slabs, int C, float *__restrict__ oa,
                                                                  float *__restrict__ ob)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float acc = 0.f;
    for (int s = 0; s < slabs; s++) acc += ws[((long)s * 2 + blockIdx.y) * C + c];
    (blockIdx.y ? ob : oa)[c] += acc;
}

// out[c] += sum over rows of x[row][c] for up to two float32 matrices of one shape (the GRU's two bias gradients: rows = T * B,
// C = D * 3H); out must hold zeros.  Workgroup = 64 columns x 4 row lanes over a slice of the rows; one float atomic per column.
__global__ __launch_bounds__(256) void colsum2_kernel(const float *__restrict__ xa, const float *__restrict__ xb, float *__restrict__ oa,
                                                      float *__restrict__ ob, long M, int C, int rows_per_block,
                                                      float *__restrict__ part /* deterministic mode: [gridDim.y][2][C] */)
{
    __shared__ float red[4][64];
    const float *x = blockIdx.z ? xb : xa;
    float *o = blockIdx.z ? ob : oa;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
    float acc = 0.f;
    if (col < C) {
        long r = r0 + rl;
        for (; r + 12 < r1; r += 16) { // four rows in flight
            const float v0 = x[r * C + col], v1 = x[(r + 4) * C + col], v2 = x[(r + 8) * C + col], v3 = x[(r + 12) * C + col];
            acc += (v0 + v1) + (v2 + v3);
        }
        for (; r < r1; r += 4) acc += x[r * C + col];
    }
    red[rl][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rl == 0 && col < C) {
        const float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (part) part[((long)blockIdx.y * 2 + blockIdx.z) * C + col] = v;
        else atomicAdd(o + col, v);
    }
}

} // namespace

// One workspace PER DEVICE (round-4 advice: a single process-global pointer, re-pointed by whichever device ran a forward last,
// made the backward kernels of device A write their slabs through device B's pointer in any single-process multi-device pattern).
// salsa_nn_set_deterministic registers the workspace for the device that is current at the call; the kernels' launchers look up
// the device current at THEIR call, so a device without a workspace keeps the atomics instead of borrowing a neighbour's.
constexpr int DET_MAX_DEV = 64;
static float *g_det_ws[DET_MAX_DEV] = {};
static size_t g_det_bytes[DET_MAX_DEV] = {};
static int det_device()
{
    int d = -1;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < DET_MAX_DEV) ? d : -1;
}
extern "C" int salsa_nn_set_deterministic(void *ws, size_t bytes)
{
    if (!ws) { // off, everywhere
        for (int i = 0; i < DET_MAX_DEV; i++) g_det_ws[i] = nullptr, g_det_bytes[i] = 0;
        return 0;
    }
    const int d = det_device();
    if (d < 0) return -6;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ws) == hipSuccess && at.type == hipMemoryTypeDevice && at.device != d) return -1; // not this device's memory
    g_det_ws[d] = (float *)ws;
    g_det_bytes[d] = bytes;
    return 0;
}
extern "C" int salsa_nn_get_deterministic(void)
{
    const int d = det_device();
    return d >= 0 && g_det_ws[d] != nullptr;
}
float *salsa_nn_det_begin(int slabs, long n, hipStream_t st, int *rc)
{
    *rc = 0;
    const int d = det_device();
    if (d < 0 || !g_det_ws[d]) return nullptr;
    const size_t need = (size_t)slabs * (size_t)n * sizeof(float);
    if (need > g_det_bytes[d]) {
        *rc = -5;
        return nullptr;
    }
    // (no clearing pass: every kernel's workgroups cover every element of their slabs -- grids are sized so that no workgroup is
    // idle -- and the GPU test runs on a NaN-poisoned workspace; a 75-MB memset per call was most of this mode's cost)
    (void)st;
    return g_det_ws[d];
}
int salsa_nn_det_finish(const float *ws, int slabs, long n, float *dw, hipStream_t st)
{
    if (slabs > 16) hipLaunchKernelGGL(slab_reduce_kernel<16>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, ws, slabs, n, dw);
    else hipLaunchKernelGGL(slab_reduce_kernel<4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, slabs, n, dw);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" {

/* out_a[c] += sum_rows a[row][c] (and out_b from b when b != NULL): float32 [M][C] row-major, the outputs must hold zeros. */
int salsa_nn_colsum2(const float *a, const float *b, float *out_a, float *out_b, int64_t M, int C, void *hip_stream)
{
    if (!a || !out_a || (b && !out_b) || M <= 0 || C <= 0) return -1;
    const int rpb = 64; // rows per workgroup: 16 per row lane
    if (M > 65535L * rpb) return -1; // ceil(M / rpb) is grid y
    const unsigned gy = (unsigned)((M + rpb - 1) / rpb);
    int rc = 0;
    float *part = salsa_nn_det_begin((int)gy, 2L * C, (hipStream_t)hip_stream, &rc);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum2_kernel, dim3((unsigned)((C + 63) / 64), gy, b ? 2u : 1u), dim3(256), 0,
                       (hipStream_t)hip_stream, a, b, out_a, out_b, (long)M, C, rpb, part);
    if (part) { // slab row = [out_a | out_b]: two strided reductions (the outputs are separate arrays)
        hipLaunchKernelGGL(slab_reduce_strided_kernel, dim3((unsigned)((C + 255) / 256), b ? 2u : 1u), dim3(256), 0, (hipStream_t)hip_stream,
                           part, (int)gy, C, out_a, out_b);
    }
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // extern "C"
