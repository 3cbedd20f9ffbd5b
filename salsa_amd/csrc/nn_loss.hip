// nn_loss.hip -- gfx950 kernels for the training losses of the SELD CRNN (C ABI: include/salsa_nn.h): the SELD loss (BCE + masked
// L1) and the ACCDOA loss (masked MSE) with their gradients, and the SED decision of the ACCDOA output.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>

#include "../../include/salsa_nn.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ SELD loss
// models/interfaces.py:304-355: sed = mean BCE-with-logits(logit, sed_gt); doa = sum over the x / y / z blocks of
// sum(|p - t| m) / sum(m) with m = sed_gt (the three blocks share sum(m)); loss = w_sed sed + w_doa doa -- and the gradients of
// sed w.r.t. logit and of doa w.r.t. the predictions (unweighted: the backward launch scales them by what flows in).
// Two launches of SELD_BLOCKS workgroups (a single 1024-thread workgroup took 64 us for the 123 k elements of a training step):
// partial sums per workgroup in float64, fixed order = deterministic; the second launch adds the partials (every workgroup for
// itself), writes the three values and the gradients of its slice.
constexpr int SELD_BLOCKS = 64;
__global__ __launch_bounds__(256) void seld_loss_partial_kernel(const float *__restrict__ logit, const float *__restrict__ doa,
                                                                const float *__restrict__ sed_gt, const float *__restrict__ doa_gt,
                                                                long rows, int nc, double *__restrict__ partial /* [SELD_BLOCKS][3] */)
{
    __shared__ double red[3][256];
    const long n = rows * nc;
    double s_bce = 0.0, s_mask = 0.0, s_abs = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)SELD_BLOCKS * 256) {
        const long r = i / nc;
        const int c = (int)(i - r * nc);
        const float x = logit[i], z = sed_gt[i];
        // max(x, 0) - x z + log1p(exp(-|x|))  (torch's binary_cross_entropy_with_logits)
        s_bce += (double)(fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x))));
        s_mask += (double)z;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) a += fabsf(doa[r * 3 * nc + k * nc + c] - doa_gt[r * 3 * nc + k * nc + c]) * z;
        s_abs += (double)a;
    }
    red[0][threadIdx.x] = s_bce;
    red[1][threadIdx.x] = s_mask;
    red[2][threadIdx.x] = s_abs;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; k++) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void seld_loss_finish_kernel(const float *__restrict__ logit, const float *__restrict__ doa,
                                                               const float *__restrict__ sed_gt, const float *__restrict__ doa_gt,
                                                               long rows, int nc, float w_sed, float w_doa,
                                                               const double *__restrict__ partial, float *__restrict__ out3,
                                                               float *__restrict__ g_logit, float *__restrict__ g_doa)
{
    __shared__ double tot[3];
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int b = 0; b < SELD_BLOCKS; b++) t += partial[b * 3 + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const long n = rows * nc;
    const float sed = (float)(tot[0] / (double)n);
    const float msum = (float)tot[1];
    const float d = (float)tot[2] / msum; // 0 / 0 = nan when no class is active anywhere, as in the reference
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out3[0] = w_sed * sed + w_doa * d;
        out3[1] = sed;
        out3[2] = d;
    }
    const float inv_n = 1.f / (float)n, inv_m = 1.f / msum;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)SELD_BLOCKS * 256) {
        const long r = i / nc;
        const int c = (int)(i - r * nc);
        const float x = logit[i], z = sed_gt[i];
        g_logit[i] = (1.f / (1.f + expf(-x)) - z) * inv_n;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long j = r * 3 * nc + k * nc + c;
            const float e = doa[j] - doa_gt[j];
            g_doa[j] = (e > 0.f ? 1.f : e < 0.f ? -1.f : 0.f) * z * inv_m;
        }
    }
}

// backward: g_logit *= g_loss w_sed + g_sed ; g_doa *= g_loss w_doa + g_doa_loss   (the incoming gradients are device scalars
// or NULL = 0), out of place
__global__ __launch_bounds__(256) void seld_loss_scale_kernel(const float *__restrict__ a, long na, const float *__restrict__ b,
                                                              long nb, const float *__restrict__ g_loss,
                                                              const float *__restrict__ g_sed, const float *__restrict__ g_d,
                                                              float w_sed, float w_doa, float *__restrict__ oa,
                                                              float *__restrict__ ob)
{
    const float gl = g_loss ? *g_loss : 0.f;
    const float fa = gl * w_sed + (g_sed ? *g_sed : 0.f), fb = gl * w_doa + (g_d ? *g_d : 0.f);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long)gridDim.x * 256) {
        if (i < na) oa[i] = a[i] * fa;
        else ob[i - na] = b[i - na] * fb;
    }
}

// ------------------------------------------------------------------------------------------------------------ ACCDOA loss
// models/interfaces.py:284-302 (compute_classwise_accdoa_loss, output_format 'accdoa'): doa = sum over (rows, class) of
// ((p_x - t_x)^2 + (p_y - t_y)^2 + (p_z - t_z)^2) m / rows with m = sed_gt; loss = doa (the reference's "sed" term is discarded).
// The gradient 2 (p - t) m / rows needs no sum: the first launch writes it (and zeros for the event logits, which the loss does
// not read) next to a float64 partial sum per workgroup; the second, one wavefront, adds the partials in a fixed order.
constexpr int ACCDOA_BLOCKS = 64;
__global__ __launch_bounds__(256) void accdoa_loss_partial_kernel(const float *__restrict__ doa, const float *__restrict__ sed_gt,
                                                                  const float *__restrict__ doa_gt, long rows, int nc,
                                                                  float *__restrict__ g_logit, float *__restrict__ g_doa,
                                                                  double *__restrict__ partial /* [ACCDOA_BLOCKS] */)
{
    __shared__ double red[256];
    const long n = rows * nc;
    const float scale = 2.f / (float)rows;
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)ACCDOA_BLOCKS * 256) {
        const long r = i / nc;
        const int c = (int)(i - r * nc);
        const float z = sed_gt[i];
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long j = r * 3 * nc + k * nc + c;
            const float e = doa[j] - doa_gt[j];
            a += e * e;
            g_doa[j] = e * z * scale;
        }
        s += (double)(a * z);
        if (g_logit) g_logit[i] = 0.f;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void accdoa_loss_finish_kernel(const double *__restrict__ partial, long rows, float *__restrict__ out3)
{
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int b = 0; b < ACCDOA_BLOCKS; b++) t += partial[b];
    const float d = (float)(t / (double)rows);
    out3[0] = d;
    out3[1] = 0.f;
    out3[2] = d;
}

// SED of the ACCDOA output (models/interfaces.py:260-268): sed[r][c] = sqrt(x^2 + y^2 + z^2) of the class's (x, y, z) in
// float32, rounded as numpy rounds it: each square, (x^2 + y^2) + z^2 and the square root correctly rounded, no fma
__global__ __launch_bounds__(256) void accdoa_sed_kernel(const float *__restrict__ xyz, float *__restrict__ sed, long rows, int nc)
{
#pragma clang fp contract(off)
    const long n = rows * nc;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / nc;
        const int c = (int)(i - r * nc);
        const float *p = xyz + r * 3 * nc + c;
        const float x = p[0], y = p[nc], z = p[2 * nc];
        sed[i] = sqrtf((x * x + y * y) + z * z); // (HIP's sqrtf is the correctly rounded one; __fsqrt_rn is native_sqrt here)
    }
}

} // namespace

extern "C" {

/* SELD training loss and its gradients (salsa_amd/crnn/loss.py; reference models/interfaces.py:304-355): logit, sed_gt
 * [rows][nc]; doa, doa_gt [rows][3 nc] float32 contiguous.  out3 = {loss, sed, doa}; g_logit / g_doa = d sed / d logit and
 * d doa / d prediction (unweighted); partial_ws: SALSA_SELD_LOSS_WS float64 values of scratch. */
int salsa_nn_seld_loss(const float *logit, const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int nc,
                       float w_sed, float w_doa, float *out3, float *g_logit, float *g_doa, double *partial_ws, void *hip_stream)
{
    if (!logit || !doa || !sed_gt || !doa_gt || !out3 || !g_logit || !g_doa || !partial_ws || rows <= 0 || nc <= 0) return -1;
    hipLaunchKernelGGL(seld_loss_partial_kernel, dim3(SELD_BLOCKS), dim3(256), 0, (hipStream_t)hip_stream, logit, doa, sed_gt, doa_gt,
                       (long)rows, nc, partial_ws);
    hipLaunchKernelGGL(seld_loss_finish_kernel, dim3(SELD_BLOCKS), dim3(256), 0, (hipStream_t)hip_stream, logit, doa, sed_gt, doa_gt,
                       (long)rows, nc, w_sed, w_doa, partial_ws, out3, g_logit, g_doa);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* out_a = a (g_loss w_sed + g_sed), out_b = b (g_loss w_doa + g_doa): the loss's backward; g_* are device scalars or NULL (= 0) */
int salsa_nn_seld_loss_bwd(const float *a, int64_t na, const float *b, int64_t nb, const float *g_loss, const float *g_sed,
                           const float *g_doa, float w_sed, float w_doa, float *out_a, float *out_b, void *hip_stream)
{
    if (!a || !b || !out_a || !out_b || na <= 0 || nb <= 0) return -1;
    const long blocks = (na + nb + 255) / 256;
    hipLaunchKernelGGL(seld_loss_scale_kernel, dim3((unsigned)(blocks < 512 ? blocks : 512)), dim3(256), 0, (hipStream_t)hip_stream, a,
                       (long)na, b, (long)nb, g_loss, g_sed, g_doa, w_sed, w_doa, out_a, out_b);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* ACCDOA training loss and its gradient (reference models/interfaces.py:273-302): sed_gt [rows][nc]; doa, doa_gt [rows][3 nc]
 * float32 contiguous.  out3 = {loss, 0, doa loss}; g_doa = d doa / d prediction; g_logit (NULL: none) [rows][nc] zero-filled;
 * partial_ws: SALSA_ACCDOA_LOSS_WS float64 values of scratch. */
int salsa_nn_accdoa_loss(const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int nc, float *out3, float *g_logit,
                         float *g_doa, double *partial_ws, void *hip_stream)
{
    if (!doa || !sed_gt || !doa_gt || !out3 || !g_doa || !partial_ws || rows <= 0 || nc <= 0) return -1;
    hipLaunchKernelGGL(accdoa_loss_partial_kernel, dim3(ACCDOA_BLOCKS), dim3(256), 0, (hipStream_t)hip_stream, doa, sed_gt, doa_gt,
                       (long)rows, nc, g_logit, g_doa, partial_ws);
    hipLaunchKernelGGL(accdoa_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (const double *)partial_ws, (long)rows,
                       out3);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* sed [rows][nc] = sqrt(x^2 + y^2 + z^2) of xyz [rows][3 nc] (blocks x | y | z), float32, bit-equal to numpy's float32 */
int salsa_nn_accdoa_sed(const float *xyz, float *sed, int64_t rows, int nc, void *hip_stream)
{
    if (!xyz || !sed || rows <= 0 || nc <= 0) return -1;
    const long blocks = (rows * nc + 255) / 256;
    hipLaunchKernelGGL(accdoa_sed_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)hip_stream, xyz,
                       sed, (long)rows, nc);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // extern "C"
