// lstm_scan.hip -- fused LSTM time scan for the SELD CRNN's lstm / bilstm decoders on gfx950 (C ABI in include/salsa_gru.h).
//
// The LSTM counterpart of gru_scan.hip's float32 streaming kernels (reference models/decoders.py: nn.LSTM(512, 256,
// num_layers=2, bidirectional=decoder_type == 'bilstm')): ONE launch per layer, a workgroup owns one (sample, direction)
// sequence, thread j owns hidden unit j, h lives in LDS and c in a register, and W_hh (1 MB fp32 per direction at H = 256) is
// streamed from L2 every step with coalesced rows.  float32 throughout, gate order i, f, g, o (PyTorch's).  There is no
// register-resident variant: 4H x H float16 at H = 256 is 512 KiB, a 1024-thread workgroup's whole register file.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_gru.h"

namespace {

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

// whh_t: [D][H(k)][4H] (weight_hh transposed by the caller): for a fixed k consecutive threads read consecutive addresses.
template <int H>
__global__ __launch_bounds__(H) void lstm_fwd_kernel(const float *__restrict__ gi, const float *__restrict__ whh_t,
                                                     const float *__restrict__ bhh, float *__restrict__ hs,
                                                     float *__restrict__ saved, int T, int B, int D)
{
    __shared__ float h[H];
    const int j = threadIdx.x;
    const int b = blockIdx.x, d = blockIdx.y;
    const float *w = whh_t + (long)d * H * 4 * H;
    const float *bb = bhh + (long)d * 4 * H;
    const float bi = bb[j], bf = bb[H + j], bg = bb[2 * H + j], bo = bb[3 * H + j];
    float cj = 0.f;
    h[j] = 0.f;
    __syncthreads();
    for (int s = 0; s < T; s++) {
        const int t = d == 0 ? s : T - 1 - s;
        const long base = ((long)t * B + b) * D + d;
        float ai = bi, af = bf, ag = bg, ao = bo;
#pragma unroll 8
        for (int k = 0; k < H; k++) {
            const float hk = h[k];
            const float *wk = w + (long)k * 4 * H;
            ai = fmaf(wk[j], hk, ai);
            af = fmaf(wk[H + j], hk, af);
            ag = fmaf(wk[2 * H + j], hk, ag);
            ao = fmaf(wk[3 * H + j], hk, ao);
        }
        const float *g = gi + base * 4 * H;
        const float ig = lstm_sigmoid(g[j] + ai);
        const float fg = lstm_sigmoid(g[H + j] + af);
        const float gg = tanhf(g[2 * H + j] + ag);
        const float og = lstm_sigmoid(g[3 * H + j] + ao);
        cj = fg * cj + ig * gg;
        const float hj = og * tanhf(cj);
        hs[base * H + j] = hj;
        if (saved) {
            float *sv = saved + base * 5 * H;
            sv[j] = ig;
            sv[H + j] = fg;
            sv[2 * H + j] = gg;
            sv[3 * H + j] = og;
            sv[4 * H + j] = cj;
        }
        __syncthreads(); // everyone has finished reading h of the previous step
        h[j] = hj;
        __syncthreads();
    }
}

// Backward scan (BPTT).  whh: [D][4H][H] PyTorch layout, so for a fixed row consecutive threads (k) read consecutive addresses
// when forming dh_prev[k] = sum_rows whh[row][k] * dg[row].  dc is carried in a register: dc_prev = dc * f; c_prev is the saved c
// of the previous scan step (zero at the first).
template <int H>
__global__ __launch_bounds__(H) void lstm_bwd_kernel(const float *__restrict__ dhs, const float *__restrict__ whh,
                                                     const float *__restrict__ saved, float *__restrict__ dg, int T, int B, int D)
{
    __shared__ float gs[4 * H];
    const int j = threadIdx.x;
    const int b = blockIdx.x, d = blockIdx.y;
    const float *w = whh + (long)d * 4 * H * H;
    float dh_carry = 0.f, dc_carry = 0.f;
    for (int s = T - 1; s >= 0; s--) { // reverse of the forward scan order
        const int t = d == 0 ? s : T - 1 - s;
        const long base = ((long)t * B + b) * D + d;
        float cprev = 0.f;
        if (s > 0) {
            const int tp = d == 0 ? t - 1 : t + 1;
            cprev = saved[(((long)tp * B + b) * D + d) * 5 * H + 4 * H + j];
        }
        const float *sv = saved + base * 5 * H;
        const float ig = sv[j], fg = sv[H + j], gg = sv[2 * H + j], og = sv[3 * H + j], c = sv[4 * H + j];
        const float tc = tanhf(c);
        const float dh = dhs[base * H + j] + dh_carry;
        const float dc = dc_carry + dh * og * (1.f - tc * tc);
        const float di_pre = dc * gg * ig * (1.f - ig);
        const float df_pre = dc * cprev * fg * (1.f - fg);
        const float dg_pre = dc * ig * (1.f - gg * gg);
        const float do_pre = dh * tc * og * (1.f - og);
        dc_carry = dc * fg;
        float *o = dg + base * 4 * H;
        o[j] = di_pre;
        o[H + j] = df_pre;
        o[2 * H + j] = dg_pre;
        o[3 * H + j] = do_pre;
        __syncthreads(); // previous step's reads of gs are done
        gs[j] = di_pre;
        gs[H + j] = df_pre;
        gs[2 * H + j] = dg_pre;
        gs[3 * H + j] = do_pre;
        __syncthreads();
        float acc = 0.f;
#pragma unroll 8
        for (int row = 0; row < 4 * H; row++) acc = fmaf(w[(long)row * H + j], gs[row], acc);
        dh_carry = acc;
    }
}

bool lstm_args_ok(int T, int B, int D, int H)
{
    return T > 0 && B > 0 && B <= 65535 && (D == 1 || D == 2) && (H == 256 || H == 128 || H == 64);
}

} // namespace

extern "C" {

int salsa_lstm_scan_fwd(const float *gi, const float *whh_t, const float *bhh, float *hs, float *saved, int T, int B, int D,
                        int H, void *hip_stream)
{
    if (!gi || !whh_t || !bhh || !hs || !lstm_args_ok(T, B, D, H)) return -1;
    hipStream_t s = (hipStream_t)hip_stream;
    dim3 grid((unsigned)B, (unsigned)D);
    if (H == 256) hipLaunchKernelGGL((lstm_fwd_kernel<256>), grid, dim3(256), 0, s, gi, whh_t, bhh, hs, saved, T, B, D);
    else if (H == 128) hipLaunchKernelGGL((lstm_fwd_kernel<128>), grid, dim3(128), 0, s, gi, whh_t, bhh, hs, saved, T, B, D);
    else hipLaunchKernelGGL((lstm_fwd_kernel<64>), grid, dim3(64), 0, s, gi, whh_t, bhh, hs, saved, T, B, D);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

int salsa_lstm_scan_bwd(const float *dhs, const float *whh, const float *saved, float *dg, int T, int B, int D, int H,
                        void *hip_stream)
{
    if (!dhs || !whh || !saved || !dg || !lstm_args_ok(T, B, D, H)) return -1;
    hipStream_t s = (hipStream_t)hip_stream;
    dim3 grid((unsigned)B, (unsigned)D);
    if (H == 256) hipLaunchKernelGGL((lstm_bwd_kernel<256>), grid, dim3(256), 0, s, dhs, whh, saved, dg, T, B, D);
    else if (H == 128) hipLaunchKernelGGL((lstm_bwd_kernel<128>), grid, dim3(128), 0, s, dhs, whh, saved, dg, T, B, D);
    else hipLaunchKernelGGL((lstm_bwd_kernel<64>), grid, dim3(64), 0, s, dhs, whh, saved, dg, T, B, D);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // extern "C"
