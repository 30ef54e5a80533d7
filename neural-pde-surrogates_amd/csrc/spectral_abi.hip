// Composite C-ABI of the spectral convolutions (include/nps.h "one call per module"): SpectralConv2d and
// SpectralConv3d forward / backward (proc_fno.py:257-288, :334-376) and the 2-D FNO layer act(conv(x) + w(x))
// (proc_fno.py:142-146), each sequencing the stage kernels of spectral.hip / spectral3d.hip on the caller's
// stream inside a caller-provided workspace.  A C caller binding libnps_hip.so needs nothing else: the weights
// are the modules' own nn.Parameters (complex64, reference layout), packed into the workspace per call.
// Host code only; every launch is stream-ordered, nothing synchronises or allocates.
#include "nps_common.hpp"

namespace {

constexpr size_t C64 = 8;  // bytes per complex64

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// Carves 256-B aligned regions out of the workspace in a fixed order (the same order the size functions sum).
struct Carve {
    char* base;
    size_t off = 0;
    float* take(size_t bytes) {
        float* p = reinterpret_cast<float*>(base + off);
        off += al256(bytes);
        return p;
    }
};

struct Spec2 {
    size_t wp, x1, x2, y, z;  // bytes of wpack [R][m2][Cin][Cout], X1 [B][H][m2][Cin], X2 [B][R][m2][Cin],
                              // Y [B][R][m2][Cout], Z [B][H][m2][Cout]
};
Spec2 spec2_sizes(int B, int Cin, int Cout, int H, int m1, int m2) {
    const size_t R = (size_t)(H < 2 * m1 ? H : 2 * m1);
    Spec2 s;
    s.wp = R * m2 * Cin * Cout * C64;
    s.x1 = (size_t)B * H * m2 * Cin * C64;
    s.x2 = (size_t)B * R * m2 * Cin * C64;
    s.y = (size_t)B * R * m2 * Cout * C64;
    s.z = (size_t)B * H * m2 * Cout * C64;
    return s;
}
// forward: [wp][X1][X2][Y][Z]; backward adds [gX2][gwp] (X1 -> gX1, Y -> gY, Z -> gZ reuse their regions)
size_t spec2_ws(int B, int Cin, int Cout, int H, int m1, int m2) {
    const Spec2 s = spec2_sizes(B, Cin, Cout, H, m1, m2);
    return al256(s.wp) + al256(s.x1) + al256(s.x2) + al256(s.y) + al256(s.z) + al256(s.x2) + al256(s.wp);
}

// FiLM operands of a composite (proc_fno.py:271-284): p [B][K], weights_feat.weight [Cout*2*m1*m2][K], its bias, and
// transform_mode.  The FiLM composites append [S][Yu][gS] to the plain workspace: the factor S [B][R][m2][Cout]
// (real), and for the backward the unscaled mixer output Yu (complex) and gS (real).
struct Film {
    const float *p, *wf, *bias;
    int K, mode;
};
// the host checks of nps_spectral_film_scale / _param_bwd (spectral.hip), made before a composite's first launch
bool film_ok(const char* what, const Film& f, int H, int m1) {
    const int R = H < 2 * m1 ? H : 2 * m1;
    if (!(f.p && f.wf && f.bias))
        nps::set_error("%s: NULL FiLM pointer (p, wf, bias)", what);
    else if (!(f.K > 0 && f.K <= 64))
        nps::set_error("%s: K (feature_transform_dim) must be in [1, 64], got %d", what, f.K);
    else if (!(f.mode == 0 || f.mode == 1))
        nps::set_error("%s: transform_mode is 0 (1 + FiLM) or 1 (FiLM), got %d", what, f.mode);
    else if (R > 32)
        nps::set_error("%s: %d retained rows > 32", what, R);
    else
        return true;
    return false;
}
size_t film_ws(int B, int Cin, int Cout, int H, int m1, int m2) {
    const Spec2 s = spec2_sizes(B, Cin, Cout, H, m1, m2);
    return spec2_ws(B, Cin, Cout, H, m1, m2) + al256(s.y / 2) + al256(s.y) + al256(s.y / 2);
}

bool spec2_args_ok(int B, int Cin, int Cout, int H, int W, int m1, int m2) {
    // proc_fno.py:134-139: modes at most the spatial dims (W // 2 + 1 for the last)
    return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && m1 > 0 && m2 > 0 && m1 <= H && m2 <= W / 2 + 1;
}

// Layout of a composite's activation operand: NHWC [B][R][W][C] (dense), or channels-first [B][C][R][W] with a batch
// stride in elements (0 = dense).  Only the W passes see it; R = H, or D*H in 3-D.
struct Lay {
    bool nchw;
    long bs;
};
constexpr Lay NHWC = {false, 0};

bool stride_ok(long bs, long per_batch) { return bs == 0 || bs >= per_batch; }

int w_dft(const nps_src_t* src, int nsrc, Lay l, int B, int R, int W, int C, int m, float* X1, void* s) {
    if (l.nchw) return nps_spectral_dft_w_nchw(src[0].ptr, l.bs, B, R, W, C, m, X1, s);
    return nps_spectral_dft_w(src, nsrc, B, R, W, C, m, X1, s);
}
int w_idft(const float* Z, float* y, Lay l, int B, int R, int W, int m, int Cout, int accumulate, int act, void* s) {
    if (l.nchw) return nps_spectral_idft_w_nchw(Z, y, l.bs, B, R, W, m, Cout, accumulate, act, s);
    return nps_spectral_idft_w(Z, y, B, R, W, m, Cout, accumulate, nullptr, act, nullptr, s);
}
int w_idft_bwd(const float* dy, Lay l, float* gZ, int B, int R, int W, int m, int Cout, void* s) {
    if (l.nchw) return nps_spectral_idft_w_bwd_nchw(dy, l.bs, gZ, B, R, W, m, Cout, s);
    return nps_spectral_idft_w_bwd(dy, gZ, B, R, W, m, Cout, s);
}
int w_dft_bwd(const float* gX1, float* dx, Lay l, int B, int R, int W, int m, int Cin, void* s) {
    if (l.nchw) return nps_spectral_dft_w_bwd_nchw(gX1, dx, l.bs, B, R, W, m, Cin, s);
    return nps_spectral_dft_w_bwd(gX1, dx, B, R, W, m, Cin, s);
}

// Z = the spectral conv up to its W-pass synthesis, for the frame `src` (nsrc sources covering B x H x W x Cin; one
// channels-first tensor when xl.nchw)
int spec2_z(const nps_src_t* src, int nsrc, Lay xl, const float* w1, const float* w2, Carve& c, const Spec2& sz, int B,
            int Cin, int Cout, int H, int W, int m1, int m2, float** Zout, float** X2out, float** wpout, void* s,
            const Film* film = nullptr, float* S = nullptr) {
    const int R = H < 2 * m1 ? H : 2 * m1;
    float* wp = c.take(sz.wp);
    float* X1 = c.take(sz.x1);
    float* X2 = c.take(sz.x2);
    float* Y = c.take(sz.y);
    float* Z = c.take(sz.z);
    int rc;
    if ((rc = nps_spectral_pack_weights(w1, w2, wp, Cin, Cout, H, m1, m2, s)) < 0) return rc;
    if ((rc = w_dft(src, nsrc, xl, B, H, W, Cin, m2, X1, s)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X1, X2, B, H, m1, m2, Cin, s)) < 0) return rc;
    if (film != nullptr) {  // Y <- Y * S in the mixer's store
        if ((rc = nps_spectral_film_scale(film->p, film->wf, film->bias, S, B, film->K, Cout, H, m1, m2, film->mode,
                                          s)) < 0)
            return rc;
        if ((rc = nps_spectral_mix_scaled(X2, wp, S, Y, B, R, m2, Cin, Cout, s)) < 0) return rc;
    } else if ((rc = nps_spectral_mix(X2, wp, Y, B, R, m2, Cin, Cout, s)) < 0) {
        return rc;
    }
    if ((rc = nps_spectral_idft_h(Y, Z, B, H, m1, m2, Cout, s)) < 0) return rc;
    *Zout = Z;
    if (X2out) *X2out = X2;
    if (wpout) *wpout = wp;
    return 0;
}

// the fused-synthesis conditions of nps_conv2d_fwd's spec_z (conv2d.hip), as a predicate
bool fno_fusable(const nps_conv2d_t& a, int m2) {
    return a.precision == NPS_PREC_X3F16 && a.KH == 1 && a.KW == 1 && a.stride == 1 && a.dil == 1 && a.Cout <= 192 &&
           !a.gn_stats && !a.pre_act && !a.accumulate && !a.addend0 && !a.addend1 && !a.out_nchw &&
           (a.out_C & 3) == 0 && (a.Cout & 3) == 0 && m2 > 0 && m2 <= 16 && (a.Wout & 127) == 0 && a.pad_y == 0 &&
           a.pad_x == 0 && a.circ == 0 && a.out_os == 1 && a.out_off_y == 0 && a.out_off_x == 0 &&
           a.out_H == a.Hout && a.out_W == a.Wout && a.nphase <= 1 && !a.s2d;
}

struct Spec3 {
    size_t wp, x1, x2, x3, y, z1, z2;
};
Spec3 spec3_sizes(int B, int Cin, int Cout, int D, int H, int m1, int m2, int m3) {
    const size_t R1 = (size_t)(D < 2 * m1 ? D : 2 * m1), R2 = (size_t)(H < 2 * m2 ? H : 2 * m2);
    Spec3 s;
    s.wp = R1 * R2 * m3 * Cin * Cout * C64;
    s.x1 = (size_t)B * D * H * m3 * Cin * C64;   // X1 [B][D*H][m3][Cin]
    s.x2 = (size_t)B * D * R2 * m3 * Cin * C64;  // X2 [B*D][R2][m3][Cin]
    s.x3 = (size_t)B * R1 * R2 * m3 * Cin * C64; // X3 [B][R1][R2*m3][Cin]
    s.y = (size_t)B * R1 * R2 * m3 * Cout * C64; // Y  [B][R1][R2*m3][Cout]
    s.z1 = (size_t)B * D * R2 * m3 * Cout * C64; // Z1 [B][D][R2*m3][Cout]
    s.z2 = (size_t)B * D * H * m3 * Cout * C64;  // Z2 [B*D][H][m3][Cout]
    return s;
}
// forward: [wp][X1][X2][X3][Y][Z1][Z2]; backward adds [gX3][gwp] (X2 -> gX2, X1 -> gX1, Y -> gY, Z1 -> gZ1,
// Z2 -> gZ2)
size_t spec3_ws(int B, int Cin, int Cout, int D, int H, int m1, int m2, int m3) {
    const Spec3 s = spec3_sizes(B, Cin, Cout, D, H, m1, m2, m3);
    return al256(s.wp) + al256(s.x1) + al256(s.x2) + al256(s.x3) + al256(s.y) + al256(s.z1) + al256(s.z2) +
           al256(s.x3) + al256(s.wp);
}
bool spec3_args_ok(int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3) {
    return B > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0 && m1 > 0 && m2 > 0 && m3 > 0 && m1 <= D &&
           m2 <= H && m3 <= W / 2 + 1;
}

}  // namespace

extern "C" size_t nps_spectral_conv2d_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2) {
    if (!spec2_args_ok(B, Cin, Cout, H, W, m1, m2)) return 0;
    return spec2_ws(B, Cin, Cout, H, m1, m2);
}

namespace {

// The 2-D composites for either layout (`what` names the entry point in the error text)
int conv2d_fwd(const char* what, const float* x, Lay xl, const float* w1, const float* w2, float* y, Lay yl, void* ws,
               int B, int Cin, int Cout, int H, int W, int m1, int m2, int accumulate, int act, void* stream,
               const Film* film = nullptr) {
    NPS_CHECK_ARG(x && w1 && w2 && y && ws, "%s: NULL pointer", what);
    if (film != nullptr && !film_ok(what, *film, H, m1)) return -1;  // before the first launch
    NPS_CHECK_ARG(spec2_args_ok(B, Cin, Cout, H, W, m1, m2),
                  "%s: modes should be at most the spatial dim (// 2 + 1 for the last spatial "
                  "dimension) (H=%d W=%d m1=%d m2=%d)", what, H, W, m1, m2);
    NPS_CHECK_ARG(act == 0 || act == 1, "%s: act is 0 (none) or 1 (GELU)", what);
    NPS_CHECK_ARG(stride_ok(xl.bs, (long)Cin * H * W) && stride_ok(yl.bs, (long)Cout * H * W),
                  "%s: a batch stride is negative or smaller than C*H*W elements (x_bs=%ld, Cin*H*W=%ld; y_bs=%ld, "
                  "Cout*H*W=%ld; 0 = dense)", what, xl.bs, (long)Cin * H * W, yl.bs, (long)Cout * H * W);
    const nps_src_t src = {x, Cin, H, W, 0, 0};
    Carve c{static_cast<char*>(ws)};
    const Spec2 sz = spec2_sizes(B, Cin, Cout, H, m1, m2);
    float* Z = nullptr;
    // the FiLM factor lies behind the plain workspace (film_ws)
    float* S = film ? reinterpret_cast<float*>(static_cast<char*>(ws) + spec2_ws(B, Cin, Cout, H, m1, m2)) : nullptr;
    int rc = spec2_z(&src, 1, xl, w1, w2, c, sz, B, Cin, Cout, H, W, m1, m2, &Z, nullptr, nullptr, stream, film, S);
    if (rc < 0) return rc;
    return w_idft(Z, y, yl, B, H, W, m2, Cout, accumulate ? 1 : 0, act, stream);
}

int conv2d_bwd(const char* what, const float* x, Lay xl, const float* w1, const float* w2, const float* dy, Lay dyl,
               float* dx, Lay dxl, float* dw1, float* dw2, void* ws, int B, int Cin, int Cout, int H, int W, int m1,
               int m2, void* stream, const Film* film = nullptr, float* dp = nullptr, float* dwf = nullptr,
               float* dbias = nullptr) {
    NPS_CHECK_ARG(x && w1 && w2 && dy && ws, "%s: NULL pointer", what);
    if (film != nullptr && !film_ok(what, *film, H, m1)) return -1;  // before the first launch
    NPS_CHECK_ARG((dw1 == nullptr) == (dw2 == nullptr), "%s: dw1 and dw2 are both given or both NULL", what);
    NPS_CHECK_ARG(spec2_args_ok(B, Cin, Cout, H, W, m1, m2), "%s: bad shape (H=%d W=%d m1=%d m2=%d)", what, H, W, m1,
                  m2);
    NPS_CHECK_ARG(stride_ok(xl.bs, (long)Cin * H * W) && stride_ok(dxl.bs, (long)Cin * H * W) &&
                      stride_ok(dyl.bs, (long)Cout * H * W),
                  "%s: a batch stride is negative or smaller than C*H*W elements (x_bs=%ld dx_bs=%ld, Cin*H*W=%ld; "
                  "dy_bs=%ld, Cout*H*W=%ld; 0 = dense)", what, xl.bs, dxl.bs, (long)Cin * H * W, dyl.bs,
                  (long)Cout * H * W);
    const int R = H < 2 * m1 ? H : 2 * m1;
    const Spec2 sz = spec2_sizes(B, Cin, Cout, H, m1, m2);
    Carve c{static_cast<char*>(ws)};
    float* wp = c.take(sz.wp);
    float* X1 = c.take(sz.x1);  // later gX1
    float* X2 = c.take(sz.x2);
    float* gY = c.take(sz.y);
    float* gZ = c.take(sz.z);
    float* gX2 = c.take(sz.x2);
    float* gwp = c.take(sz.wp);
    float* S = film ? c.take(sz.y / 2) : nullptr;  // FiLM only (film_ws)
    float* Yu = film ? c.take(sz.y) : nullptr;
    float* gS = film ? c.take(sz.y / 2) : nullptr;
    const nps_src_t src = {x, Cin, H, W, 0, 0};
    int rc;
    // the forward's retained spectrum X2 (mix_bwd's conj(X2) for the weight gradient) and the packed weight
    if ((rc = nps_spectral_pack_weights(w1, w2, wp, Cin, Cout, H, m1, m2, stream)) < 0) return rc;
    if ((rc = w_dft(&src, 1, xl, B, H, W, Cin, m2, X1, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X1, X2, B, H, m1, m2, Cin, stream)) < 0) return rc;
    // adjoint chain: irfft2's adjoint, the H pass, the mixing's two adjoint products
    if ((rc = w_idft_bwd(dy, dyl, gZ, B, H, W, m2, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(gZ, gY, B, H, m1, m2, Cout, stream)) < 0) return rc;
    if (film != nullptr) {
        // the factor and the unscaled mixer output again (never Y / S: S may be zero); gS from them, gY <- gY * S
        if ((rc = nps_spectral_film_scale(film->p, film->wf, film->bias, S, B, film->K, Cout, H, m1, m2, film->mode,
                                          stream)) < 0)
            return rc;
        if ((rc = nps_spectral_mix(X2, wp, Yu, B, R, m2, Cin, Cout, stream)) < 0) return rc;
        if ((rc = nps_spectral_film_bwd(Yu, S, gY, gS, B, R, m2, Cout, stream)) < 0) return rc;
        if (dp != nullptr || dwf != nullptr || dbias != nullptr)
            if ((rc = nps_spectral_film_param_bwd(gS, film->p, film->wf, dwf, dbias, dp, B, film->K, Cout, H, m1, m2,
                                                  film->mode, stream)) < 0)
                return rc;
    }
    if ((rc = nps_spectral_mix_bwd(X2, wp, gY, gX2, gwp, B, R, m2, Cin, Cout, stream)) < 0) return rc;
    if (dx != nullptr) {
        if ((rc = nps_spectral_idft_h(gX2, X1, B, H, m1, m2, Cin, stream)) < 0) return rc;
        if ((rc = w_dft_bwd(X1, dx, dxl, B, H, W, m2, Cin, stream)) < 0) return rc;
    }
    if (dw1 != nullptr)
        if ((rc = nps_spectral_unpack_grad(gwp, dw1, dw2, Cin, Cout, H, m1, m2, stream)) < 0) return rc;
    return 0;
}

}  // namespace

extern "C" int nps_spectral_conv2d_fwd(const float* x, const float* w1, const float* w2, float* y, void* ws, int B,
                                       int Cin, int Cout, int H, int W, int m1, int m2, int accumulate, int act,
                                       void* stream) {
    return conv2d_fwd("spectral_conv2d_fwd", x, NHWC, w1, w2, y, NHWC, ws, B, Cin, Cout, H, W, m1, m2, accumulate, act,
                      stream);
}

extern "C" int nps_spectral_conv2d_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, float* y,
                                            long y_bs, void* ws, int B, int Cin, int Cout, int H, int W, int m1,
                                            int m2, int accumulate, int act, void* stream) {
    return conv2d_fwd("spectral_conv2d_fwd_nchw", x, Lay{true, x_bs}, w1, w2, y, Lay{true, y_bs}, ws, B, Cin, Cout, H,
                      W, m1, m2, accumulate, act, stream);
}

extern "C" int nps_spectral_conv2d_bwd(const float* x, const float* w1, const float* w2, const float* dy, float* dx,
                                       float* dw1, float* dw2, void* ws, int B, int Cin, int Cout, int H, int W,
                                       int m1, int m2, void* stream) {
    return conv2d_bwd("spectral_conv2d_bwd", x, NHWC, w1, w2, dy, NHWC, dx, NHWC, dw1, dw2, ws, B, Cin, Cout, H, W, m1,
                      m2, stream);
}

extern "C" int nps_spectral_conv2d_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2,
                                            const float* dy, long dy_bs, float* dx, long dx_bs, float* dw1,
                                            float* dw2, void* ws, int B, int Cin, int Cout, int H, int W, int m1,
                                            int m2, void* stream) {
    return conv2d_bwd("spectral_conv2d_bwd_nchw", x, Lay{true, x_bs}, w1, w2, dy, Lay{true, dy_bs}, dx,
                      Lay{true, dx_bs}, dw1, dw2, ws, B, Cin, Cout, H, W, m1, m2, stream);
}

extern "C" size_t nps_spectral_conv2d_film_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2) {
    if (!spec2_args_ok(B, Cin, Cout, H, W, m1, m2)) return 0;
    return film_ws(B, Cin, Cout, H, m1, m2);
}

extern "C" int nps_spectral_conv2d_film_fwd(const float* x, const float* w1, const float* w2, const float* p,
                                            const float* wf, const float* bias, float* y, void* ws, int B, int Cin,
                                            int Cout, int H, int W, int m1, int m2, int K, int transform_mode,
                                            int accumulate, int act, void* stream) {
    const Film f = {p, wf, bias, K, transform_mode};
    return conv2d_fwd("spectral_conv2d_film_fwd", x, NHWC, w1, w2, y, NHWC, ws, B, Cin, Cout, H, W, m1, m2, accumulate,
                      act, stream, &f);
}

extern "C" int nps_spectral_conv2d_film_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2,
                                                 const float* p, const float* wf, const float* bias, float* y,
                                                 long y_bs, void* ws, int B, int Cin, int Cout, int H, int W, int m1,
                                                 int m2, int K, int transform_mode, int accumulate, int act,
                                                 void* stream) {
    const Film f = {p, wf, bias, K, transform_mode};
    return conv2d_fwd("spectral_conv2d_film_fwd_nchw", x, Lay{true, x_bs}, w1, w2, y, Lay{true, y_bs}, ws, B, Cin,
                      Cout, H, W, m1, m2, accumulate, act, stream, &f);
}

extern "C" int nps_spectral_conv2d_film_bwd(const float* x, const float* w1, const float* w2, const float* p,
                                            const float* wf, const float* bias, const float* dy, float* dx, float* dw1,
                                            float* dw2, float* dp, float* dwf, float* dbias, void* ws, int B, int Cin,
                                            int Cout, int H, int W, int m1, int m2, int K, int transform_mode,
                                            void* stream) {
    const Film f = {p, wf, bias, K, transform_mode};
    return conv2d_bwd("spectral_conv2d_film_bwd", x, NHWC, w1, w2, dy, NHWC, dx, NHWC, dw1, dw2, ws, B, Cin, Cout, H, W,
                      m1, m2, stream, &f, dp, dwf, dbias);
}

extern "C" int nps_spectral_conv2d_film_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2,
                                                 const float* p, const float* wf, const float* bias, const float* dy,
                                                 long dy_bs, float* dx, long dx_bs, float* dw1, float* dw2, float* dp,
                                                 float* dwf, float* dbias, void* ws, int B, int Cin, int Cout, int H,
                                                 int W, int m1, int m2, int K, int transform_mode, void* stream) {
    const Film f = {p, wf, bias, K, transform_mode};
    return conv2d_bwd("spectral_conv2d_film_bwd_nchw", x, Lay{true, x_bs}, w1, w2, dy, Lay{true, dy_bs}, dx,
                      Lay{true, dx_bs}, dw1, dw2, ws, B, Cin, Cout, H, W, m1, m2, stream, &f, dp, dwf, dbias);
}

extern "C" size_t nps_fno_layer2d_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2) {
    return nps_spectral_conv2d_workspace(B, Cin, Cout, H, W, m1, m2);
}

extern "C" int nps_fno_layer2d_fwd(const nps_conv2d_t* w, const float* w1, const float* w2, int m1, int m2, void* ws,
                                   void* stream) {
    NPS_CHECK_ARG(w && w1 && w2 && ws, "fno_layer2d_fwd: NULL pointer");
    const nps_conv2d_t& a = *w;
    NPS_CHECK_ARG(a.KH == 1 && a.KW == 1 && a.stride == 1 && a.dil == 1 && a.Hout == a.Hin && a.Wout == a.Win &&
                      a.spec_z == nullptr && !a.accumulate,
                  "fno_layer2d_fwd: w is the layer's 1x1 conv over the whole frame (no accumulate, spec_z unset)");
    NPS_CHECK_ARG(a.act == 0 || a.act == 1, "fno_layer2d_fwd: act is 0 (none) or 1 (GELU)");
    const int B = a.B, Cin = a.Cin, Cout = a.Cout, H = a.Hin, W = a.Win;
    NPS_CHECK_ARG(spec2_args_ok(B, Cin, Cout, H, W, m1, m2), "fno_layer2d_fwd: bad modes (H=%d W=%d m1=%d m2=%d)", H,
                  W, m1, m2);
    Carve c{static_cast<char*>(ws)};
    const Spec2 sz = spec2_sizes(B, Cin, Cout, H, m1, m2);
    float* Z = nullptr;
    int rc = spec2_z(a.src, a.nsrc, NHWC, w1, w2, c, sz, B, Cin, Cout, H, W, m1, m2, &Z, nullptr, nullptr, stream);
    if (rc < 0) return rc;
    nps_conv2d_t f = a;
    if (fno_fusable(a, m2)) {
        // one output pass: the 1x1's epilogue synthesises the c2r W pass (1 / (H W), irfft2's norm), then act
        f.spec_z = Z;
        f.spec_m2 = m2;
        f.spec_scale = 1.0f / ((float)H * (float)W);
        return nps_conv2d_fwd(&f, stream);
    }
    // w(x) + bias without the activation, then y = act(y + c2r(Z) / (H W)) in the idft_w pass
    NPS_CHECK_ARG(!a.out_nchw && a.out_C == Cout && a.out_H == H && a.out_W == W && a.out_os == 1 && a.out_off_y == 0 &&
                      a.out_off_x == 0 && !a.addend0 && !a.addend1 && a.out_stats == nullptr,
                  "fno_layer2d_fwd: the unfused synthesis needs a dense NHWC [B][H][W][Cout] output, no addend / "
                  "out_stats");
    f.act = 0;
    if ((rc = nps_conv2d_fwd(&f, stream)) < 0) return rc;
    return nps_spectral_idft_w(Z, a.out, B, H, W, m2, Cout, 1, nullptr, a.act, a.out_tag, stream);
}

extern "C" size_t nps_spectral_conv3d_workspace(int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3) {
    if (!spec3_args_ok(B, Cin, Cout, D, H, W, m1, m2, m3)) return 0;
    return spec3_ws(B, Cin, Cout, D, H, m1, m2, m3);
}

namespace {

int conv3d_fwd(const char* what, const float* x, Lay xl, const float* w1, const float* w2, const float* w3,
               const float* w4, float* y, Lay yl, void* ws, int B, int Cin, int Cout, int D, int H, int W, int m1,
               int m2, int m3, int accumulate, int act, void* stream) {
    NPS_CHECK_ARG(x && w1 && w2 && w3 && w4 && y && ws, "%s: NULL pointer", what);
    NPS_CHECK_ARG(spec3_args_ok(B, Cin, Cout, D, H, W, m1, m2, m3),
                  "%s: modes should be at most the spatial dim (// 2 + 1 for the last spatial "
                  "dimension) (D=%d H=%d W=%d m=%d,%d,%d)", what, D, H, W, m1, m2, m3);
    NPS_CHECK_ARG(act == 0 || act == 1, "%s: act is 0 (none) or 1 (GELU)", what);
    NPS_CHECK_ARG(stride_ok(xl.bs, (long)Cin * D * H * W) && stride_ok(yl.bs, (long)Cout * D * H * W),
                  "%s: a batch stride is negative or smaller than C*D*H*W elements (x_bs=%ld, Cin*D*H*W=%ld; "
                  "y_bs=%ld, Cout*D*H*W=%ld; 0 = dense)", what, xl.bs, (long)Cin * D * H * W, yl.bs,
                  (long)Cout * D * H * W);
    const int R1 = D < 2 * m1 ? D : 2 * m1, R2 = H < 2 * m2 ? H : 2 * m2;
    const Spec3 sz = spec3_sizes(B, Cin, Cout, D, H, m1, m2, m3);
    Carve c{static_cast<char*>(ws)};
    float* wp = c.take(sz.wp);
    float* X1 = c.take(sz.x1);
    float* X2 = c.take(sz.x2);
    float* X3 = c.take(sz.x3);
    float* Y = c.take(sz.y);
    float* Z1 = c.take(sz.z1);
    float* Z2 = c.take(sz.z2);
    const nps_src_t src = {x, Cin, D * H, W, 0, 0};  // NDHWC viewed as (B, D*H, W, C); NCDHW as (B, C, D*H, W)
    int rc;
    if ((rc = nps_spectral3d_pack_weights(w1, w2, w3, w4, wp, Cin, Cout, D, H, m1, m2, m3, stream)) < 0) return rc;
    if ((rc = w_dft(&src, 1, xl, B, D * H, W, Cin, m3, X1, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X1, X2, B * D, H, m2, m3, Cin, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X2, X3, B, D, m1, R2 * m3, Cin, stream)) < 0) return rc;
    if ((rc = nps_spectral_mix(X3, wp, Y, B, R1, R2 * m3, Cin, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_idft_h(Y, Z1, B, D, m1, R2 * m3, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_idft_h(Z1, Z2, B * D, H, m2, m3, Cout, stream)) < 0) return rc;
    return w_idft(Z2, y, yl, B, D * H, W, m3, Cout, accumulate ? 1 : 0, act, stream);
}

int conv3d_bwd(const char* what, const float* x, Lay xl, const float* w1, const float* w2, const float* w3,
               const float* w4, const float* dy, Lay dyl, float* dx, Lay dxl, float* dw1, float* dw2, float* dw3,
               float* dw4, void* ws, int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3,
               void* stream) {
    NPS_CHECK_ARG(x && w1 && w2 && w3 && w4 && dy && ws, "%s: NULL pointer", what);
    const bool gw = dw1 != nullptr;
    NPS_CHECK_ARG((dw2 != nullptr) == gw && (dw3 != nullptr) == gw && (dw4 != nullptr) == gw,
                  "%s: dw1..dw4 are all given or all NULL", what);
    NPS_CHECK_ARG(spec3_args_ok(B, Cin, Cout, D, H, W, m1, m2, m3), "%s: bad shape", what);
    NPS_CHECK_ARG(stride_ok(xl.bs, (long)Cin * D * H * W) && stride_ok(dxl.bs, (long)Cin * D * H * W) &&
                      stride_ok(dyl.bs, (long)Cout * D * H * W),
                  "%s: a batch stride is negative or smaller than C*D*H*W elements (x_bs=%ld dx_bs=%ld, "
                  "Cin*D*H*W=%ld; dy_bs=%ld, Cout*D*H*W=%ld; 0 = dense)", what, xl.bs, dxl.bs, (long)Cin * D * H * W,
                  dyl.bs, (long)Cout * D * H * W);
    const int R1 = D < 2 * m1 ? D : 2 * m1, R2 = H < 2 * m2 ? H : 2 * m2;
    const Spec3 sz = spec3_sizes(B, Cin, Cout, D, H, m1, m2, m3);
    Carve c{static_cast<char*>(ws)};
    float* wp = c.take(sz.wp);
    float* X1 = c.take(sz.x1);   // later gX1
    float* X2 = c.take(sz.x2);   // later gX2
    float* X3 = c.take(sz.x3);
    float* gY = c.take(sz.y);
    float* gZ1 = c.take(sz.z1);
    float* gZ2 = c.take(sz.z2);
    float* gX3 = c.take(sz.x3);
    float* gwp = c.take(sz.wp);
    const nps_src_t src = {x, Cin, D * H, W, 0, 0};
    int rc;
    if ((rc = nps_spectral3d_pack_weights(w1, w2, w3, w4, wp, Cin, Cout, D, H, m1, m2, m3, stream)) < 0) return rc;
    if ((rc = w_dft(&src, 1, xl, B, D * H, W, Cin, m3, X1, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X1, X2, B * D, H, m2, m3, Cin, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(X2, X3, B, D, m1, R2 * m3, Cin, stream)) < 0) return rc;
    if ((rc = w_idft_bwd(dy, dyl, gZ2, B, D * H, W, m3, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(gZ2, gZ1, B * D, H, m2, m3, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_dft_h(gZ1, gY, B, D, m1, R2 * m3, Cout, stream)) < 0) return rc;
    if ((rc = nps_spectral_mix_bwd(X3, wp, gY, gX3, gwp, B, R1, R2 * m3, Cin, Cout, stream)) < 0) return rc;
    if (dx != nullptr) {
        if ((rc = nps_spectral_idft_h(gX3, X2, B, D, m1, R2 * m3, Cin, stream)) < 0) return rc;
        if ((rc = nps_spectral_idft_h(X2, X1, B * D, H, m2, m3, Cin, stream)) < 0) return rc;
        if ((rc = w_dft_bwd(X1, dx, dxl, B, D * H, W, m3, Cin, stream)) < 0) return rc;
    }
    if (gw)
        if ((rc = nps_spectral3d_unpack_grad(gwp, dw1, dw2, dw3, dw4, Cin, Cout, D, H, m1, m2, m3, stream)) < 0)
            return rc;
    return 0;
}

}  // namespace

extern "C" int nps_spectral_conv3d_fwd(const float* x, const float* w1, const float* w2, const float* w3,
                                       const float* w4, float* y, void* ws, int B, int Cin, int Cout, int D, int H,
                                       int W, int m1, int m2, int m3, int accumulate, int act, void* stream) {
    return conv3d_fwd("spectral_conv3d_fwd", x, NHWC, w1, w2, w3, w4, y, NHWC, ws, B, Cin, Cout, D, H, W, m1, m2, m3,
                      accumulate, act, stream);
}

extern "C" int nps_spectral_conv3d_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2,
                                            const float* w3, const float* w4, float* y, long y_bs, void* ws, int B,
                                            int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3,
                                            int accumulate, int act, void* stream) {
    return conv3d_fwd("spectral_conv3d_fwd_nchw", x, Lay{true, x_bs}, w1, w2, w3, w4, y, Lay{true, y_bs}, ws, B, Cin,
                      Cout, D, H, W, m1, m2, m3, accumulate, act, stream);
}

extern "C" int nps_spectral_conv3d_bwd(const float* x, const float* w1, const float* w2, const float* w3,
                                       const float* w4, const float* dy, float* dx, float* dw1, float* dw2,
                                       float* dw3, float* dw4, void* ws, int B, int Cin, int Cout, int D, int H, int W,
                                       int m1, int m2, int m3, void* stream) {
    return conv3d_bwd("spectral_conv3d_bwd", x, NHWC, w1, w2, w3, w4, dy, NHWC, dx, NHWC, dw1, dw2, dw3, dw4, ws, B,
                      Cin, Cout, D, H, W, m1, m2, m3, stream);
}

extern "C" int nps_spectral_conv3d_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2,
                                            const float* w3, const float* w4, const float* dy, long dy_bs, float* dx,
                                            long dx_bs, float* dw1, float* dw2, float* dw3, float* dw4, void* ws,
                                            int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3,
                                            void* stream) {
    return conv3d_bwd("spectral_conv3d_bwd_nchw", x, Lay{true, x_bs}, w1, w2, w3, w4, dy, Lay{true, dy_bs}, dx,
                      Lay{true, dx_bs}, dw1, dw2, dw3, dw4, ws, B, Cin, Cout, D, H, W, m1, m2, m3, stream);
}
