/*
 * salsa_gru.h -- C ABI of the fused GRU scan used by the SELD CRNN consumer (models/decoders.py:44-46 in the upstream
 * repo: nn.GRU(512, 256, num_layers=2, bidirectional=True)).  One launch runs the whole time recurrence of one layer
 * for every (sample, direction) pair; the input projections W_ih x + b_ih are one dense GEMM done by the caller.
 * All tensors are float32, device pointers, caller-owned; asynchronous on the given HIP stream.  The LSTM scans at the end
 * (salsa_amd/csrc/lstm_scan.hip) serve the decoder_type lstm / bilstm decoders the same way.
 *
 *   gi    [T][B][D][3H]  input projections, gate order r,z,n (PyTorch's)
 *   whh   [D][3H][H]     weight_hh (PyTorch layout, row = gate*H + unit); whh_t [D][H][3H] is its transpose per direction
 *   bhh   [D][3H]
 *   hs    [T][B][D][H]   hidden state AFTER step t (direction 1 scans t = T-1..0 and still stores at index t)
 *   saved [T][B][D][4H]  r, z, n, (W_hn h + b_hn) per step, for the backward scan (may be NULL for inference)
 *
 * Every entry point checks its arguments on the host before any launch and returns -1 for T <= 0, B outside 1..65535, D outside
 * {1, 2}, an H it has no instantiation for (64, 128, 256; the register-resident pair: 256) or a NULL among the required pointers.
 */
#ifndef SALSA_GRU_H
#define SALSA_GRU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int salsa_gru_scan_fwd(const float *gi, const float *whh_t, const float *bhh, float *hs, float *saved, int T, int B, int D,
                       int H, void *hip_stream);

/* Register-resident variants for H = 256: the recurrent weights (PyTorch layout whh, rounded to float16) stay in the
 * registers of a 1024-thread workgroup for the whole scan instead of being streamed from L2 every step; float32 state,
 * gates and accumulation.  Used without gradients (saved = NULL) and for training under bf16 autocast, where the backward
 * variant differentiates the same rounded weights (same arguments as salsa_gru_scan_bwd). */
int salsa_gru_scan_fwd_regw(const float *gi, const float *whh, const float *bhh, float *hs, float *saved, int T, int B, int D,
                            int H, void *hip_stream);
int salsa_gru_scan_bwd_regw(const float *dhs, const float *whh, const float *hs, const float *saved, float *dgi, float *dgh,
                            int T, int B, int D, int H, void *hip_stream);

/* dhs [T][B][D][H] = gradient wrt every hs[t].  Outputs: dgi [T][B][D][3H] (gradient wrt gi) and dgh [T][B][D][3H]
 * (gradient wrt W_hh h_prev + b_hh; the caller forms dW_hh = sum_t,b dgh^T h_prev and db_hh with one GEMM). */
int salsa_gru_scan_bwd(const float *dhs, const float *whh, const float *hs, const float *saved, float *dgi, float *dgh,
                       int T, int B, int D, int H, void *hip_stream);

/* LSTM (gate order i, f, g, o: PyTorch's), float32 streaming scans, H in {64, 128, 256}, D in {1, 2}; one workgroup per
 * (sample, direction), one thread per hidden unit, h in LDS, c in a register, W_hh streamed from L2 every step.
 *
 *   gi    [T][B][D][4H]  input projections W_ih x + b_ih
 *   whh_t [D][H][4H]     weight_hh transposed per direction (forward); whh [D][4H][H] PyTorch layout (backward)
 *   bhh   [D][4H]
 *   hs    [T][B][D][H]   hidden state AFTER step t (direction 1 scans t = T-1..0 and still stores at index t)
 *   saved [T][B][D][5H]  i, f, g, o (activated) and c per step, for the backward scan (NULL: inference)
 *
 * _bwd: dhs [T][B][D][H] = gradient wrt every hs[t] -> dg [T][B][D][4H], the gradient wrt the gate pre-activations, which is
 * both the gradient wrt gi and wrt W_hh h_prev + b_hh (the caller forms dW_hh = sum_t,b dg^T h_prev and db_ih = db_hh =
 * colsum(dg)).  Both return 0, -1 for invalid arguments, -6 when the launch fails. */
int salsa_lstm_scan_fwd(const float *gi, const float *whh_t, const float *bhh, float *hs, float *saved, int T, int B, int D,
                        int H, void *hip_stream);
int salsa_lstm_scan_bwd(const float *dhs, const float *whh, const float *saved, float *dg, int T, int B, int D, int H,
                        void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
