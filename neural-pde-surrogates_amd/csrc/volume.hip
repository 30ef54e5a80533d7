// approx_volume_preserve modes 'block' and 'individual' (activation_wrapper.py:40-79), forward and backward.
//
// Every mode is out[b,c,t] = u[b,c,t] * F[b,c,t] (+ the re-applied spatial-cond mask), with F a function of the
// plane totals s_t = sum_hw u[b,c,t] and p = sum_hw x[b,c,-1] only.  The totals arrive as fp64 (nps_plane_sums), so
// the factor kernels keep every scalar in fp64: one thread per (b, c) walks the time window.  That is B * c threads
// x tw steps, nothing next to the passes over u, and it keeps the cancelling 1 - s/p (then divided by
// max_pct_dif / 100) out of fp32.  The element-wise passes are fp32 and take F (and the backward's per-plane
// constant c) as one fp32 scalar per plane.
#include "nps_common.hpp"

#include <cstdint>

namespace {

constexpr int FACTOR_THREADS = 64;
constexpr int APPLY_THREADS = 256;

// F[bc][t], fp64 scalars.  k = 100 / max_pct_dif; r(s, p) = 1 - tanh((1 - s / p) k) / k.
//   block:      Sm = mean_t s_t;  F_t = p r(Sm, p) / Sm for every t
//   individual: p_0 = p;  r_i = r(s_i, p_i);  F_i = r_i p_i / s_i;  p_{i+1} = r_i p_i
__global__ void volume_factors_kernel(const double* __restrict__ new_tot, const double* __restrict__ prev_tot,
                                      int mode, double k, int nbc, int tw, float* __restrict__ F) {
    const int bc = blockIdx.x * blockDim.x + threadIdx.x;
    if (bc >= nbc) return;
    const double* s = new_tot + (size_t)bc * tw;
    float* f = F + (size_t)bc * tw;
    double p = prev_tot[bc];
    if (mode == NPS_VOLUME_BLOCK) {
        double sm = 0.0;
        for (int t = 0; t < tw; ++t) sm += s[t];
        sm /= tw;
        const double r = 1.0 - tanh((1.0 - sm / p) * k) / k;
        const float fb = (float)(p * r / sm);
        for (int t = 0; t < tw; ++t) f[t] = fb;
    } else {
        for (int i = 0; i < tw; ++i) {
            const double q = (1.0 - tanh((1.0 - s[i] / p) * k) / k) * p;  // r_i p_i
            f[i] = (float)(q / s[i]);
            p = q;
        }
    }
}

// c[bc][t] = sum_t' D_t' dF_t' / ds_t, fp64 scalars (D_t = sum_hw g (1 - mask) u: nps_plane_dot).
//   block:      th = tanh((1 - Sm / p) k);  c_t = (sum_t' D_t') ((1 - th^2) / Sm - p r / Sm^2) / tw for every t
//   individual: with q_i = r_i p_i (so F_i = q_i / s_i, dq_i/ds_i = 1 - th_i^2, dq_i/dp_i = r_i - (1 - th_i^2) s_i / p_i)
//               the forward recurrence is recomputed into ws[bc][i] = p_i, then from i = tw - 1 down, lambda = 0:
//                 a = D_i / s_i + lambda;  c_i = -D_i q_i / s_i^2 + a (1 - th_i^2);  lambda = a dq_i/dp_i
__global__ void volume_factors_bwd_kernel(const double* __restrict__ new_tot, const double* __restrict__ prev_tot,
                                          const double* __restrict__ D, int mode, double k, int nbc, int tw,
                                          double* __restrict__ ws, float* __restrict__ c) {
    const int bc = blockIdx.x * blockDim.x + threadIdx.x;
    if (bc >= nbc) return;
    const double* s = new_tot + (size_t)bc * tw;
    const double* d = D + (size_t)bc * tw;
    float* co = c + (size_t)bc * tw;
    double p = prev_tot[bc];
    if (mode == NPS_VOLUME_BLOCK) {
        double sm = 0.0, dsum = 0.0;
        for (int t = 0; t < tw; ++t) {
            sm += s[t];
            dsum += d[t];
        }
        sm /= tw;
        const double th = tanh((1.0 - sm / p) * k);
        const double r = 1.0 - th / k;
        const float cb = (float)(dsum * ((1.0 - th * th) / sm - p * r / (sm * sm)) / tw);
        for (int t = 0; t < tw; ++t) co[t] = cb;
    } else {
        double* ps = ws + (size_t)bc * tw;
        for (int i = 0; i < tw; ++i) {
            ps[i] = p;
            p = (1.0 - tanh((1.0 - s[i] / p) * k) / k) * p;
        }
        double lambda = 0.0;
        for (int i = tw - 1; i >= 0; --i) {
            const double pi = ps[i], si = s[i];
            const double th = tanh((1.0 - si / pi) * k);
            const double r = 1.0 - th / k;
            const double sech2 = 1.0 - th * th;
            const double a = d[i] / si + lambda;
            co[i] = (float)(-d[i] * r * pi / (si * si) + a * sech2);
            lambda = a * (r - sech2 * si / pi);
        }
    }
}

// u[plane] *= F[plane], then v -= mask v, in place.  grid (blocks per plane, planes), grid-stride within the plane;
// VEC: HW % 4 == 0 and every base 16-byte aligned, so each plane is a whole number of aligned float4.
template <bool VEC>
__global__ void volume_apply_kernel(float* __restrict__ u, const float* __restrict__ F,
                                    const float* __restrict__ mask, int mask_S, int mask_ch, int nct, int HW) {
    const int plane = blockIdx.y;  // (b, c, t)
    const int b = plane / nct;
    const float f = F[plane];
    float* pl = u + (size_t)plane * HW;
    const float* mk = mask ? mask + ((size_t)b * mask_S + mask_ch) * HW : nullptr;
    const int step = gridDim.x * blockDim.x;
    if (VEC) {
        f32x4* pl4 = reinterpret_cast<f32x4*>(pl);
        const f32x4* mk4 = reinterpret_cast<const f32x4*>(mk);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW / 4; i += step) {
            f32x4 v = pl4[i] * f;
            if (mk) v = v - mk4[i] * v;
            pl4[i] = v;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += step) {
            float v = pl[i] * f;
            if (mk) v = v - mk[i] * v;
            pl[i] = v;
        }
    }
}

// gu[plane] = g (1 - mask) F[plane] + c[plane]; the launch shape of volume_apply_kernel
template <bool VEC>
__global__ void volume_apply_bwd_kernel(const float* __restrict__ g, const float* __restrict__ F,
                                        const float* __restrict__ c, const float* __restrict__ mask, int mask_S,
                                        int mask_ch, int nct, int HW, float* __restrict__ gu) {
    const int plane = blockIdx.y;
    const int b = plane / nct;
    const float f = F[plane], cc = c[plane];
    const float* gp = g + (size_t)plane * HW;
    float* op = gu + (size_t)plane * HW;
    const float* mk = mask ? mask + ((size_t)b * mask_S + mask_ch) * HW : nullptr;
    const int step = gridDim.x * blockDim.x;
    if (VEC) {
        const f32x4* gp4 = reinterpret_cast<const f32x4*>(gp);
        const f32x4* mk4 = reinterpret_cast<const f32x4*>(mk);
        f32x4* op4 = reinterpret_cast<f32x4*>(op);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW / 4; i += step) {
            f32x4 gg = gp4[i];
            if (mk) gg = gg - mk4[i] * gg;
            op4[i] = gg * f + cc;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += step) {
            float gg = gp[i];
            if (mk) gg = gg - mk[i] * gg;
            op[i] = gg * f + cc;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks per plane: one float4 (or four floats) per thread up to 64 blocks, grid-stride beyond
inline int apply_blocks(int HW) {
    const int nb = (HW + APPLY_THREADS * 4 - 1) / (APPLY_THREADS * 4);
    return nb < 1 ? 1 : (nb > 64 ? 64 : nb);
}

}  // namespace

#define NPS_VOLUME_CHECK_WINDOW(what)                                                                              \
    NPS_CHECK_ARG(B > 0 && num_c > 0 && tw > 0, what ": non-positive extent (B=%d num_c=%d tw=%d)", B, num_c, tw); \
    NPS_CHECK_ARG((long)B * num_c * tw <= 65535, what ": B * num_c * tw = %ld planes exceed the 65535 of a launch", \
                  (long)B * num_c * tw)

#define NPS_VOLUME_CHECK_MODE(what)                                                                           \
    NPS_CHECK_ARG(mode == NPS_VOLUME_BLOCK || mode == NPS_VOLUME_INDIVIDUAL, what ": unknown mode %d", mode); \
    NPS_CHECK_ARG(std::isfinite(max_pct_dif) && max_pct_dif > 0.0,                                            \
                  what ": max_pct_dif %g is not finite and positive", max_pct_dif)

extern "C" int nps_volume_factors(const double* new_tot, const double* prev_tot, int mode, double max_pct_dif,
                                  float* F, int B, int num_c, int tw, void* stream) {
    NPS_CHECK_ARG(new_tot && prev_tot && F, "volume_factors: null pointer");
    NPS_VOLUME_CHECK_WINDOW("volume_factors");
    NPS_VOLUME_CHECK_MODE("volume_factors");
    const int nbc = B * num_c;
    volume_factors_kernel<<<(nbc + FACTOR_THREADS - 1) / FACTOR_THREADS, FACTOR_THREADS, 0, (hipStream_t)stream>>>(
        new_tot, prev_tot, mode, 100.0 / max_pct_dif, nbc, tw, F);
    NPS_CHECK_LAUNCH("volume_factors");
    return 0;
}

extern "C" int nps_volume_factors_bwd(const double* new_tot, const double* prev_tot, const double* D, int mode,
                                      double max_pct_dif, double* ws, float* c, int B, int num_c, int tw,
                                      void* stream) {
    NPS_CHECK_ARG(new_tot && prev_tot && D && c, "volume_factors_bwd: null pointer");
    NPS_VOLUME_CHECK_WINDOW("volume_factors_bwd");
    NPS_VOLUME_CHECK_MODE("volume_factors_bwd");
    NPS_CHECK_ARG(mode != NPS_VOLUME_INDIVIDUAL || ws, "volume_factors_bwd: null pointer (ws, mode 'individual')");
    const int nbc = B * num_c;
    volume_factors_bwd_kernel<<<(nbc + FACTOR_THREADS - 1) / FACTOR_THREADS, FACTOR_THREADS, 0,
                                (hipStream_t)stream>>>(new_tot, prev_tot, D, mode, 100.0 / max_pct_dif, nbc, tw, ws,
                                                       c);
    NPS_CHECK_LAUNCH("volume_factors_bwd");
    return 0;
}

extern "C" int nps_volume_apply(float* u, const float* F, const float* mask, int mask_S, int mask_ch, int B,
                                int num_c, int tw, int H, int W, void* stream) {
    NPS_CHECK_ARG(u && F, "volume_apply: null pointer");
    NPS_VOLUME_CHECK_WINDOW("volume_apply");
    NPS_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= 0x3fffffff, "volume_apply: bad plane extent (H=%d W=%d)", H, W);
    NPS_CHECK_ARG(!mask || (mask_ch >= 0 && mask_ch < mask_S), "volume_apply: mask_ch %d outside the mask's %d channels",
                  mask_ch, mask_S);
    const int HW = H * W;
    const dim3 grid(apply_blocks(HW), B * num_c * tw);
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(u) && aligned16(mask))
        volume_apply_kernel<true><<<grid, APPLY_THREADS, 0, s>>>(u, F, mask, mask_S, mask_ch, num_c * tw, HW);
    else
        volume_apply_kernel<false><<<grid, APPLY_THREADS, 0, s>>>(u, F, mask, mask_S, mask_ch, num_c * tw, HW);
    NPS_CHECK_LAUNCH("volume_apply");
    return 0;
}

extern "C" int nps_volume_apply_bwd(const float* g, const float* F, const float* c, const float* mask, int mask_S,
                                    int mask_ch, float* gu, int B, int num_c, int tw, int H, int W, void* stream) {
    NPS_CHECK_ARG(g && F && c && gu, "volume_apply_bwd: null pointer");
    NPS_VOLUME_CHECK_WINDOW("volume_apply_bwd");
    NPS_CHECK_ARG(H > 0 && W > 0 && (long)H * W <= 0x3fffffff, "volume_apply_bwd: bad plane extent (H=%d W=%d)", H, W);
    NPS_CHECK_ARG(!mask || (mask_ch >= 0 && mask_ch < mask_S),
                  "volume_apply_bwd: mask_ch %d outside the mask's %d channels", mask_ch, mask_S);
    const int HW = H * W;
    const dim3 grid(apply_blocks(HW), B * num_c * tw);
    hipStream_t s = (hipStream_t)stream;
    if (HW % 4 == 0 && aligned16(g) && aligned16(gu) && aligned16(mask))
        volume_apply_bwd_kernel<true><<<grid, APPLY_THREADS, 0, s>>>(g, F, c, mask, mask_S, mask_ch, num_c * tw, HW, gu);
    else
        volume_apply_bwd_kernel<false><<<grid, APPLY_THREADS, 0, s>>>(g, F, c, mask, mask_S, mask_ch, num_c * tw, HW,
                                                                      gu);
    NPS_CHECK_LAUNCH("volume_apply_bwd");
    return 0;
}
