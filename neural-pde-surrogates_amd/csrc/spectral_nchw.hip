// Channels-first W passes of the spectral convolutions (proc_fno.py:257-288, :334-376): the reference's
// SpectralConv2d / SpectralConv3d take and return (B, C, H, W) / (B, C, D, H, W).  Only the two W passes touch
// the activations, so these two kernels are all a channels-first caller needs; X1 / Z and every stage between
// them keep the layouts of spectral.hip.  A tensor is viewed as [B][C][R][W] (R = H, or D*H in 3-D): W
// contiguous, plane stride R*W, and an explicit batch stride (elements) so a channel slice of a larger tensor is
// passed without a copy.  Every global access is a dword with lanes along w (x / out) or along c (X1 / Z): full
// 256-B wave runs at any 4-byte alignment, so there is no vector path and no alignment condition to dispatch on.
#include "nps_common.hpp"

namespace {

// (cos theta, sin theta), theta = 2 pi k n / N, from the exact integer phase
__device__ __forceinline__ float2 twiddle(int k, int n, int N) {
    const int ph = (int)(((long)k * n) % N);
    float s, c;
    sincospif(2.0f * (float)ph / (float)N, &s, &c);
    return make_float2(c, s);
}

inline int kc_for(int m2) { return m2 <= 4 ? 4 : (m2 <= 8 ? 8 : (m2 <= 12 ? 12 : 16)); }

constexpr int AW = 32;      // pixels per LDS chunk of the analysis
constexpr int AP = AW + 1;  // tile row pitch: lane c reads tile[c][w] at stride 33 dwords, conflict-free (ds_read_b32
                            // banks are dword % 32 per 32-lane half)
constexpr size_t A_TILES = 4 * 32 * AP * sizeof(float);  // one [32][AP] tile per wave
constexpr size_t A_LDS_MAX = 128 * 1024;

// X1[b][r][k][c] = f_k sum_w x[b][c][r][w] e^{-2 pi i k w / W}   (scale / c2r_adj as dft_w_kernel of spectral.hip)
// The exact-fp32 MFMA GEMM of dft_w_mfma_kernel, X1[k][c] = sum_w T[k][w] x[w][c] with M = [cos | sin] rows of 16 bins,
// N = 32 channels, K = 2 pixels per v_mfma_f32_32x32x2_f32 in ascending w (the same fmaf chain as the NHWC kernel for
// even W).  A wave owns (row, 32-channel tile): it loads 32-pixel runs of two channels per instruction (lanes along
// w), transposes them through its LDS tile and reads the B operand with lanes along c.  The next chunk's loads are
// in flight during the MFMAs.  Pixels past W and channels past C are zero in the tile, bins past m2 zero in the
// table, so odd W and any C take the same path; more than 16 bins run as passes of 16 over the same table space.
__global__ __launch_bounds__(256) void dft_w_nchw_kernel(const float* __restrict__ x, long bs, int R, int W, int C,
                                                         int m2, float2* __restrict__ X1, float scale, int c2r_adj,
                                                         int nrows, int Wp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // twm [Wp][32] | tiles [4][32][AP]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
    float* twm = lds;
    float* tile = lds + (size_t)Wp * 32 + wave * 32 * AP;
    const int ntile = (C + 31) / 32;
    const long ntask = (long)nrows * ntile;
    const long plane = (long)R * W;
    for (int kb = 0; kb < m2; kb += 16) {
        __syncthreads();
        for (int i = threadIdx.x; i < Wp * 32; i += 256) {
            const int w = i >> 5, m = i & 31;
            const int k = kb + (m & 15);
            float v = 0.f;
            if (k < m2 && w < W) {
                const float2 t = twiddle(k, w, W);
                v = m < 16 ? t.x : t.y;
            }
            twm[i] = v;
        }
        __syncthreads();
        for (long t0 = (long)blockIdx.x * 4; t0 < ntask; t0 += (long)gridDim.x * 4) {  // uniform trip count per WG
            const long task = t0 + wave;
            const bool valid = task < ntask;
            const int row = (int)(task / ntile), c0 = (int)(task - (long)row * ntile) * 32;
            const int b = row / R, r = row - b * R;
            const float* src = x + (long)b * bs + (long)c0 * plane + (long)r * W;
            float pre[16];
            auto fetch = [&](int w0) {
                const int w = w0 + l32;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 2 * i + h;
                    pre[i] = (valid && c0 + c < C && w < W) ? src[(long)c * plane + w] : 0.f;
                }
            };
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            fetch(0);
            for (int w0 = 0; w0 < Wp; w0 += AW) {
                __syncthreads();  // the tile's previous readers are done
#pragma unroll
                for (int i = 0; i < 16; ++i) tile[(2 * i + h) * AP + l32] = pre[i];
                __syncthreads();
                if (w0 + AW < Wp) fetch(w0 + AW);
#pragma unroll
                for (int u = 0; u < AW / 2; ++u) {
                    const float t = twm[(w0 + 2 * u + h) * 32 + l32];
                    const float xv = tile[l32 * AP + 2 * u + h];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t, xv, acc, 0, 0, 0);
                }
            }
            // accumulator lane l, register q: column l % 32, row 8 (q / 4) + 4 (l / 32) + q % 4; cos row k, sin row 16 + k
            const int c = c0 + l32;
            if (valid && c < C) {
                float2* dst = X1 + (size_t)row * m2 * C + c;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int k = kb + 8 * (q >> 2) + 4 * h + (q & 3);
                    if (k < m2) {
                        float f = scale;
                        if (c2r_adj && !((k == 0) || (2 * k == W))) f *= 2.f;
                        dst[(size_t)k * C] = make_float2(acc[q] * f, -acc[q + 8] * f);
                    }
                }
            }
        }
    }
}

constexpr int OT = 64;  // output channels per staged Z tile of the synthesis

// out[b][o][r][w] (=|+=) act(scale sum_k c_k Re(Z[b][r][k][o] e^{+2 pi i k w / W}))   (semantics of idft_w_kernel)
// A work-group takes `rpb` consecutive (b, r) rows; a lane owns PX pixels (w = tid + j * blockDim) and keeps their
// (cos, sin) of the KC bins of a pass in registers across the rows.  Per row and 64-channel tile the Z values are
// staged in LDS as [KC / 2][64] float4 = bins (2q, 2q + 1) of channel o with the c2r multipliers applied (DC and even-W
// Nyquist once with Im dropped, the others doubled when `doubling`); the lane then walks o reading them as broadcast
// ds_read_b128 and runs the fmaf order of idft_w_kernel's pixel().  Loads of the previous value and stores are
// coalesced along w.  More than 16 bins run as passes over out, as in the NHWC kernel.
template <int KC, int PX>
__global__ __launch_bounds__(256) void idft_w_nchw_kernel(const float2* __restrict__ Z, float* __restrict__ out,
                                                          long bs, int R, int W, int m2, int Cout, int nrows, int rpb,
                                                          int accumulate, int act, float scale, int doubling) {
    __shared__ f32x4 zs[(KC / 2) * OT];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int row0 = blockIdx.x * rpb, row1 = min(row0 + rpb, nrows);
    const long plane = (long)R * W;
    for (int wt = 0; wt < W; wt += PX * nt) {
        int wj[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) wj[j] = wt + tid + j * nt;
        for (int kb = 0; kb < m2; kb += KC) {
            const int nk = min(KC, m2 - kb);
            float tc[PX][KC], ts[PX][KC];
#pragma unroll
            for (int j = 0; j < PX; ++j)
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    float2 t = make_float2(0.f, 0.f);
                    if (k < nk && wj[j] < W) t = twiddle(kb + k, wj[j], W);
                    tc[j][k] = t.x;
                    ts[j][k] = t.y;
                }
            const bool last_chunk = kb + KC >= m2;
            const bool rd_out = kb > 0 || accumulate;
            for (int row = row0; row < row1; ++row) {
                const int b = row / R, r = row - b * R;
                float* orow = out + (long)b * bs + (long)r * W;
                const float2* zrow = Z + (size_t)row * m2 * Cout;
                for (int o0 = 0; o0 < Cout; o0 += OT) {
                    __syncthreads();
                    for (int i = tid; i < (KC / 2) * OT; i += nt) {
                        const int q = i / OT, o = o0 + (i - q * OT);
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int k = 2 * q + e, kk = kb + k;
                            if (k < nk && o < Cout) {
                                const float2 z = zrow[(size_t)kk * Cout + o];
                                const bool self_conj = (kk == 0) || (2 * kk == W);
                                const float cm = (self_conj || !doubling) ? 1.f : 2.f;
                                v[2 * e] = z.x * cm;
                                v[2 * e + 1] = self_conj ? 0.f : z.y * cm;
                            }
                        }
                        zs[i] = v;
                    }
                    __syncthreads();
                    const int no = min(OT, Cout - o0);
#pragma unroll 2
                    for (int oo = 0; oo < no; ++oo) {
                        float* p = orow + (long)(o0 + oo) * plane;
                        float prev[PX], v[PX];
#pragma unroll
                        for (int j = 0; j < PX; ++j) {
                            prev[j] = (rd_out && wj[j] < W) ? p[wj[j]] : 0.f;
                            v[j] = 0.f;
                        }
#pragma unroll
                        for (int q = 0; q < KC / 2; ++q) {
                            const f32x4 t = zs[q * OT + oo];  // (re, im) of bins 2q, 2q + 1
#pragma unroll
                            for (int j = 0; j < PX; ++j) {
                                v[j] = fmaf(t[0], tc[j][2 * q], fmaf(-t[1], ts[j][2 * q], v[j]));
                                v[j] = fmaf(t[2], tc[j][2 * q + 1], fmaf(-t[3], ts[j][2 * q + 1], v[j]));
                            }
                        }
#pragma unroll
                        for (int j = 0; j < PX; ++j) {
                            float y = kb == 0 ? (accumulate ? v[j] * scale + prev[j] : v[j] * scale)
                                              : prev[j] + v[j] * scale;
                            if (last_chunk && act == 1) y = nps::gelu_erf(y);
                            if (wj[j] < W) p[wj[j]] = y;
                        }
                    }
                }
            }
        }
    }
}

int cu_count() {
    static int ncu = 0;
    if (ncu == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        ncu = n;
    }
    return ncu;
}

// 0 = dense; otherwise at least one batch's C*R*W elements
bool stride_ok(long bs, int C, int R, int W) { return bs == 0 || bs >= (long)C * R * W; }
long stride_of(long bs, int C, int R, int W) { return bs == 0 ? (long)C * R * W : bs; }

int launch_analysis(const char* what, const float* x, long bs, int B, int R, int W, int C, int m2, float* X1,
                    float scale, int c2r_adj, hipStream_t s) {
    const int Wp = (W + AW - 1) / AW * AW;
    const size_t lds = (size_t)Wp * 32 * sizeof(float) + A_TILES;
    NPS_CHECK_ARG(lds <= A_LDS_MAX, "%s: W=%d too large (the twiddle table needs %zu B of LDS)", what, W, lds);
    NPS_CHECK_ARG((long)B * R <= 0x7fffffffL, "%s: B*rows=%ld too large", what, (long)B * R);
    if (lds > 64 * 1024) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute((const void*)dft_w_nchw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)A_LDS_MAX);
            attr_set = true;
        }
    }
    const int nrows = B * R;
    const long groups = ((long)nrows * ((C + 31) / 32) + 3) / 4;
    const int g = (int)(groups < 2L * cu_count() ? groups : 2L * cu_count());  // persistent: the table is built once
    dft_w_nchw_kernel<<<g, 256, lds, s>>>(x, stride_of(bs, C, R, W), R, W, C, m2, reinterpret_cast<float2*>(X1), scale,
                                          c2r_adj, nrows, Wp);
    return 0;
}

template <int KC>
void launch_synthesis_kc(int g, int nt, int px, hipStream_t s, const float2* Z, float* out, long bs, int R, int W,
                         int m2, int C, int nrows, int rpb, int accumulate, int act, float scale, int doubling) {
    if (px == 2)
        idft_w_nchw_kernel<KC, 2><<<g, nt, 0, s>>>(Z, out, bs, R, W, m2, C, nrows, rpb, accumulate, act, scale,
                                                    doubling);
    else
        idft_w_nchw_kernel<KC, 1><<<g, nt, 0, s>>>(Z, out, bs, R, W, m2, C, nrows, rpb, accumulate, act, scale,
                                                    doubling);
}

int launch_synthesis(const char* what, const float* Z, float* out, long bs, int B, int R, int W, int m2, int C,
                     int accumulate, int act, float scale, int doubling, hipStream_t s) {
    NPS_CHECK_ARG((long)B * R <= 0x7fffffffL, "%s: B*rows=%ld too large", what, (long)B * R);
    const int nrows = B * R;
    const int px = W > 64 ? 2 : 1;  // two pixels per lane halve the LDS reads per FMA once a wave is full
    const int per = (W + px - 1) / px;
    const int nt = per >= 256 ? 256 : (per + 63) / 64 * 64;
    // rows per work-group: amortise the lane's twiddles while leaving >= 8 work-groups per CU
    int rpb = nrows / (8 * cu_count());
    rpb = rpb < 1 ? 1 : (rpb > 8 ? 8 : rpb);
    const int g = (nrows + rpb - 1) / rpb;
    const float2* z = reinterpret_cast<const float2*>(Z);
    const long obs = stride_of(bs, C, R, W);
    switch (kc_for(m2)) {
        case 4: launch_synthesis_kc<4>(g, nt, px, s, z, out, obs, R, W, m2, C, nrows, rpb, accumulate, act, scale, doubling); break;
        case 8: launch_synthesis_kc<8>(g, nt, px, s, z, out, obs, R, W, m2, C, nrows, rpb, accumulate, act, scale, doubling); break;
        case 12: launch_synthesis_kc<12>(g, nt, px, s, z, out, obs, R, W, m2, C, nrows, rpb, accumulate, act, scale, doubling); break;
        default: launch_synthesis_kc<16>(g, nt, px, s, z, out, obs, R, W, m2, C, nrows, rpb, accumulate, act, scale, doubling); break;
    }
    return 0;
}

}  // namespace

#define NPS_NCHW_SHAPE(what, C)                                                                                  \
    NPS_CHECK_ARG(B > 0 && H > 0 && W > 0 && (C) > 0 && m2 > 0 && m2 <= W / 2 + 1, what ": bad shape (B=%d H=%d W=%d " \
                  "C=%d m2=%d; m2 <= W / 2 + 1)", B, H, W, (C), m2)
#define NPS_NCHW_STRIDE(what, bs, C)                                                                              \
    NPS_CHECK_ARG(stride_ok((bs), (C), H, W), what ": batch stride %ld is negative or smaller than C*H*W = %ld "  \
                  "elements (0 = dense)", (long)(bs), (long)(C) * H * W)

extern "C" int nps_spectral_dft_w_nchw(const float* x, long x_bs, int B, int H, int W, int C, int m2, float* X1,
                                       void* stream) {
    NPS_CHECK_ARG(x && X1, "spectral_dft_w_nchw: NULL pointer");
    NPS_NCHW_SHAPE("spectral_dft_w_nchw", C);
    NPS_NCHW_STRIDE("spectral_dft_w_nchw", x_bs, C);
    int rc = launch_analysis("spectral_dft_w_nchw", x, x_bs, B, H, W, C, m2, X1, 1.f, 0, (hipStream_t)stream);
    if (rc < 0) return rc;
    NPS_CHECK_LAUNCH("spectral_dft_w_nchw");
    return 0;
}

extern "C" int nps_spectral_idft_w_nchw(const float* Z, float* out, long out_bs, int B, int H, int W, int m2, int Cout,
                                        int accumulate, int act, void* stream) {
    NPS_CHECK_ARG(Z && out, "spectral_idft_w_nchw: NULL pointer");
    NPS_NCHW_SHAPE("spectral_idft_w_nchw", Cout);
    NPS_NCHW_STRIDE("spectral_idft_w_nchw", out_bs, Cout);
    NPS_CHECK_ARG(act == 0 || act == 1, "spectral_idft_w_nchw: act is 0 (none) or 1 (GELU)");
    int rc = launch_synthesis("spectral_idft_w_nchw", Z, out, out_bs, B, H, W, m2, Cout, accumulate ? 1 : 0, act,
                              1.0f / ((float)H * (float)W), 1, (hipStream_t)stream);
    if (rc < 0) return rc;
    NPS_CHECK_LAUNCH("spectral_idft_w_nchw");
    return 0;
}

extern "C" int nps_spectral_idft_w_bwd_nchw(const float* gy, long gy_bs, float* gZ, int B, int H, int W, int m2,
                                            int Cout, void* stream) {
    NPS_CHECK_ARG(gy && gZ, "spectral_idft_w_bwd_nchw: NULL pointer");
    NPS_NCHW_SHAPE("spectral_idft_w_bwd_nchw", Cout);
    NPS_NCHW_STRIDE("spectral_idft_w_bwd_nchw", gy_bs, Cout);
    int rc = launch_analysis("spectral_idft_w_bwd_nchw", gy, gy_bs, B, H, W, Cout, m2, gZ,
                             1.0f / ((float)H * (float)W), 1, (hipStream_t)stream);
    if (rc < 0) return rc;
    NPS_CHECK_LAUNCH("spectral_idft_w_bwd_nchw");
    return 0;
}

extern "C" int nps_spectral_dft_w_bwd_nchw(const float* gX1, float* gx, long gx_bs, int B, int H, int W, int m2,
                                           int Cin, void* stream) {
    NPS_CHECK_ARG(gX1 && gx, "spectral_dft_w_bwd_nchw: NULL pointer");
    NPS_NCHW_SHAPE("spectral_dft_w_bwd_nchw", Cin);
    NPS_NCHW_STRIDE("spectral_dft_w_bwd_nchw", gx_bs, Cin);
    int rc = launch_synthesis("spectral_dft_w_bwd_nchw", gX1, gx, gx_bs, B, H, W, m2, Cin, 0, 0, 1.0f, 0,
                              (hipStream_t)stream);
    if (rc < 0) return rc;
    NPS_CHECK_LAUNCH("spectral_dft_w_bwd_nchw");
    return 0;
}
