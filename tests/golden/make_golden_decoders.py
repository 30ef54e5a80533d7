"""Generate the grid-decoder fixtures (tests/golden/decoders_*.pt) from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (make_golden.REF_SRC) and stores plain
tensors only.  Nothing on the GPU box or in the product path runs it.

Every case builds the reference's real module under torch.manual_seed(42), runs it on the CPU in fp32 and, from a copy
cast to float64 (complex parameters to complex128 by hand), in fp64, each under the same random cotangent g.

decoders_mod_<case>.pt  one record per case of the four decoder classes of dec_grid.py on their own, h (B, hidden, *spatial)
    and u (B, c, tw, *spatial) in, around a stub pde (dt):
      cls, kwargs (the constructor's, without pde and activation), dt, beta (TimeConv: set on its Swish), state_dict,
      h, u, g, y64, gh64 (gradient of h), grads64 {parameter: gradient},
      e_ref {"y" / "h" / parameter: rel-L2 of the reference's own fp32 result against fp64}
decoders_epd_<name>.pt  EncProcDec(enc_grid.ElementWise / FNO / each decoder) on an 8 x 12 grid, B = 2, one FNO layer
    of 2 x 2 modes, hidden 16 (32 for TimeConv), n_cond_static = 1, n_cond_spatial = 1; `wrapped` cases go through
    activation_wrapper(Tanh, enforce_spatial_cond=True):
      kwargs, pde, wrapper (or None), state_dict, x, cond, pos, spatial_cond, g, y64, e_ref
decoders_epd_<name>_grads.pt  {parameter: fp64 gradient} of that case.

Usage (from any cwd):  python tests/golden/make_golden_decoders.py
"""
import copy
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_stubs, REF_SRC  # noqa: E402

B = 2
LIMIT = 200 * 1000
# name: (class, constructor kwargs, spatial, dt)
MODULES = {
    "tcl_2d": ("TimeConvLinear", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=16), (5, 6), 0.3),
    "tcl_tw1_all": ("TimeConvLinear", dict(num_c=3, num_spatial_dims=2, time_window=1, hidden_features=16,
                                           dec_delta_mode="all"), (5, 6), 0.3),
    "tcl_tw4_1d_none": ("TimeConvLinear", dict(num_c=1, num_spatial_dims=1, time_window=4, hidden_features=16,
                                               dec_delta_mode="none"), (13,), 0.3),
    "tcl_3d_nodt": ("TimeConvLinear", dict(num_c=2, num_spatial_dims=3, time_window=8, hidden_features=16,
                                           dec_delta_dt=False), (3, 4, 5), 0.3),
    "tc_h32": ("TimeConv", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=32), (5, 6), 0.3),
    "tc_h48_all": ("TimeConv", dict(num_c=1, num_spatial_dims=2, time_window=4, hidden_features=48,
                                    dec_delta_mode="all"), (5, 6), 0.3),
    "tc_h16_1d_none": ("TimeConv", dict(num_c=2, num_spatial_dims=1, time_window=5, hidden_features=16,
                                        dec_delta_mode="none"), (13,), 0.3),
    "tc_h128_beta": ("TimeConv", dict(num_c=3, num_spatial_dims=2, time_window=25, hidden_features=128), (3, 4), 0.1),
    "tc_h32_3d": ("TimeConv", dict(num_c=1, num_spatial_dims=3, time_window=5, hidden_features=32), (3, 4, 5), 0.3),
    "tcd_all": ("TimeConvDense", dict(num_c=2, num_spatial_dims=2, time_window=8, hidden_features=16,
                                      dec_delta_mode="all"), (5, 6), 0.3),
    "tcd_none_3d": ("TimeConvDense", dict(num_c=3, num_spatial_dims=3, time_window=25, hidden_features=16,
                                          dec_delta_mode="none"), (2, 3, 5), 0.1),
    "tcd_per_step": ("TimeConvDense", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=16), (5, 6),
                     0.3),
    "lc_k3_circ": ("LinearConv", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=16,
                                      dec_kernel_size=3, dec_padding_mode="circular"), (7, 9), 0.3),
    "lc_k1_zeros_all": ("LinearConv", dict(num_c=2, num_spatial_dims=2, time_window=5, hidden_features=16,
                                           dec_kernel_size=1, dec_padding_mode="zeros", dec_delta_mode="all"), (7, 9),
                        0.3),
    "lc_1d_k3_none": ("LinearConv", dict(num_c=2, num_spatial_dims=1, time_window=5, hidden_features=16,
                                         dec_kernel_size=3, dec_padding_mode="zeros", dec_delta_mode="none"), (13,),
                      0.3),
    "lc_3d": ("LinearConv", dict(num_c=1, num_spatial_dims=3, time_window=2, hidden_features=4, dec_kernel_size=3,
                                 dec_padding_mode="zeros"), (3, 4, 5), 0.3),
}
BETA = {"tc_h128_beta": 0.5}

EPD_COMMON = dict(encoder="enc_grid.ElementWise", processor="FNO", num_spatial_dims=2, hidden_blocks=1, fno_modes=2,
                  cond_mode="concat", fno_kernel_size=1, fno_conv_mode="single")
EPD_PDE = dict(dt=0.3, n_cond_static=1, n_cond_spatial=1)
EPD_GRID = (8, 12)
WRAP = dict(enforce_spatial_cond=True, spatial_cond_channel=0)
EPD = {
    "tcl": (dict(EPD_COMMON, decoder="dec_grid.TimeConvLinear", num_c=2, time_window=5, hidden_features=16), None),
    "tc": (dict(EPD_COMMON, decoder="dec_grid.TimeConv", num_c=2, time_window=5, hidden_features=32,
                dec_delta_mode="all"), None),
    "tcd_none": (dict(EPD_COMMON, decoder="dec_grid.TimeConvDense", num_c=2, time_window=8, hidden_features=16,
                      dec_delta_mode="none"), None),
    "lc": (dict(EPD_COMMON, decoder="dec_grid.LinearConv", num_c=2, time_window=5, hidden_features=16,
                dec_kernel_size=3, dec_padding_mode="circular"), None),
    "tcl_wrapped": (dict(EPD_COMMON, decoder="dec_grid.TimeConvLinear", num_c=2, time_window=5, hidden_features=16),
                    WRAP),
}


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    from torch import nn
    torch.set_num_threads(8)
    import models
    from models.enc_proc_dec import EncProcDec
    from models.enc_proc_dec_components import dec_grid

    gen = torch.Generator().manual_seed(31415)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    def to64(m):
        m64 = copy.deepcopy(m).double()
        for p in m64.parameters():
            if p.is_complex():
                p.data = p.data.to(torch.complex128)
        return m64

    def rel(a, b):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        return (torch.linalg.vector_norm(a.double() - b.double()) / torch.linalg.vector_norm(b.double())).item()

    def save(fname, payload):
        path = os.path.join(HERE, fname)
        torch.save(payload, path)
        size = os.path.getsize(path)
        assert size < LIMIT, (fname, size)
        print(f"  wrote {fname}  ({size / 1000:.1f} kB)")

    out = {}
    for name, (cls, kw, spatial, dt) in MODULES.items():
        torch.manual_seed(42)
        extra = {} if cls in ("TimeConv", "LinearConv") else dict(activation=nn.GELU())
        m = getattr(dec_grid, cls)(pde=types.SimpleNamespace(dt=dt), **kw, **extra)
        if name in BETA:
            m.decoder[1].beta = BETA[name]
        h = rnd(B, kw["hidden_features"], *spatial).requires_grad_(True)
        u = rnd(B, kw["num_c"], kw["time_window"], *spatial, lo=0.0, hi=1.0)
        y32 = m(h, u)
        g = rnd(*y32.shape)
        y32.backward(g)
        m64 = to64(m)
        h64 = h.detach().double().requires_grad_(True)
        y64 = m64(h64, u.double())
        y64.backward(g.double())
        g64 = {k: p.grad.detach().clone() for k, p in m64.named_parameters()}
        assert all(v.abs().max() > 0 for v in g64.values())
        e_ref = {k: rel(p.grad, g64[k]) for k, p in m.named_parameters()}
        e_ref["y"], e_ref["h"] = rel(y32.detach(), y64.detach()), rel(h.grad, h64.grad)
        out[name] = dict(cls=cls, kwargs=dict(kw), dt=dt, beta=BETA.get(name, 1.0),
                         state_dict={k: v.detach().clone() for k, v in m.state_dict().items()}, h=h.detach().clone(),
                         u=u, g=g, y64=y64.detach().clone(), gh64=h64.grad.detach().clone(), grads64=g64, e_ref=e_ref)
        print(f"{name}: e_ref y {e_ref['y']:.2e} h {e_ref['h']:.2e} worst parameter "
              f"{max(v for k, v in e_ref.items() if k not in ('y', 'h')):.2e}")
        save(f"decoders_mod_{name}.pt", out.pop(name))

    for name, (kw, wrapper) in EPD.items():
        pde = types.SimpleNamespace(**EPD_PDE)
        torch.manual_seed(42)
        if wrapper is None:
            m = EncProcDec(pde=pde, activation=nn.GELU(), **kw)
        else:
            m = models.activation_wrapper(model_class="EncProcDec", activation_final=nn.Tanh(), pde=pde,
                                          activation=nn.GELU(), **wrapper, **kw)
        H, W = EPD_GRID
        x = rnd(B, kw["num_c"], kw["time_window"], H, W, lo=0.0, hi=1.0)
        cond = rnd(B, pde.n_cond_static, lo=0.0, hi=1.0)
        axes = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        pos = torch.stack(axes, dim=-1)[None].repeat(B, 1, 1, 1).contiguous()
        sc = (rnd(B, 1, H, W, lo=0.0, hi=1.0) > 0.8).float()
        call = lambda mod, c: mod(x=c(x), cond=c(cond), bc=None, pos=c(pos), t_cond=None, spatial_cond=c(sc))  # noqa: E731
        y32 = call(m, lambda t: t)
        g = rnd(*y32.shape)
        y32.backward(g)
        m64 = to64(m)
        y64 = call(m64, lambda t: t.double())
        y64.backward(g.double())
        g64 = {k: p.grad.detach().clone() for k, p in m64.named_parameters()}
        assert all(v.abs().max() > 0 for v in g64.values())
        e_ref = {k: rel(p.grad, g64[k]) for k, p in m.named_parameters()}
        e_ref["y"] = rel(y32.detach(), y64.detach())
        rec = dict(kwargs=dict(kw), pde=dict(EPD_PDE), wrapper=wrapper,
                   state_dict={k: v.detach().clone() for k, v in m.state_dict().items()}, x=x, cond=cond, pos=pos,
                   spatial_cond=sc, g=g, y64=y64.detach().clone(), e_ref=e_ref)
        print(f"epd {name}: e_ref y {e_ref['y']:.2e} worst parameter "
              f"{max(v for k, v in e_ref.items() if k != 'y'):.2e}")
        save(f"decoders_epd_{name}.pt", rec)
        save(f"decoders_epd_{name}_grads.pt", g64)


if __name__ == "__main__":
    main()
