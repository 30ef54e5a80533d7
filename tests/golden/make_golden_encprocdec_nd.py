"""Generate the 1-D / 3-D EncProcDec fixture (tests/golden/encprocdec_nd.pt) from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (make_golden.REF_SRC) and stores plain
tensors only — seeded state_dicts, inputs, outputs and the reference's own autograd gradients.  Nothing on the GPU
box or in the product path runs it.

Two cases from the reference's real EncProcDec (enc_proc_dec.py:41-183) with encoder="enc_grid.ElementWise",
decoder="dec_grid.TimeConvDense", activation=nn.GELU(), processor="FNO", hidden_features=16, hidden_blocks=2,
cond_mode="concat", each constructed under torch.manual_seed(42) around a stub pde (dt, n_cond_static,
n_cond_spatial — all the grid path reads):
  epd1d_fno: num_spatial_dims=1, num_c=2, time_window=5 (decoder kernels 3 / 3, L1 = 7), L = 72, fno_modes=5,
      n_cond_static=2, B=2, pos passed as (B, L)
  epd3d_fno: num_spatial_dims=3, num_c=1, time_window=25, (D, H, W) = (4, 6, 10), fno_modes=(3, 4, 3),
      n_cond_static=3, n_cond_spatial=1 with spatial_cond (B, 1, D, H, W), B=2
The stub dt is large (0.5 / 0.1) so that the decoder's delta, not the copied last input step, makes up most of y.
Every case records kwargs, pde, state_dict, x, cond, pos, spatial_cond (3-D), y, a random cotangent g and the
gradient of every parameter.

The 3-D FNO's spectral weights are 4 x (20, 16, 3, 4, 3) complex64 per layer: 720 KiB for the two layers, and as
much again for their gradients.  No committed file may exceed 1 MiB, so the 3-D case's gradients go to a second file,
encprocdec_nd_grads3d.pt ({"epd3d_fno": {name: grad}}); everything else is in encprocdec_nd.pt.

Usage (from any cwd):  python tests/golden/make_golden_encprocdec_nd.py
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_stubs, REF_SRC  # noqa: E402

COMMON = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", processor="FNO", hidden_features=16,
              hidden_blocks=2, cond_mode="concat")
CASES = {
    "epd1d_fno": dict(kwargs=dict(COMMON, num_spatial_dims=1, num_c=2, time_window=5, fno_modes=5),
                      pde=dict(dt=0.5, n_cond_static=2, n_cond_spatial=0), spatial=(72,), B=2),
    "epd3d_fno": dict(kwargs=dict(COMMON, num_spatial_dims=3, num_c=1, time_window=25, fno_modes=(3, 4, 3)),
                      pde=dict(dt=0.1, n_cond_static=3, n_cond_spatial=1), spatial=(4, 6, 10), B=2),
}


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    from torch import nn
    torch.set_num_threads(8)
    from models.enc_proc_dec import EncProcDec

    gen = torch.Generator().manual_seed(2718)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    out, big = {}, {}
    for name, case in CASES.items():
        kw, spatial, B = case["kwargs"], case["spatial"], case["B"]
        nd = len(spatial)
        pde = types.SimpleNamespace(**case["pde"])
        torch.manual_seed(42)
        m = EncProcDec(pde=pde, activation=nn.GELU(), **kw)
        x = rnd(B, kw["num_c"], kw["time_window"], *spatial, lo=0.0, hi=1.0)
        cond = rnd(B, pde.n_cond_static, lo=0.0, hi=1.0)
        axes = torch.meshgrid(*[torch.linspace(0, 1, s) for s in spatial], indexing="ij")
        pos = torch.stack(axes, dim=-1)[None].repeat(B, *([1] * (nd + 1))).contiguous()
        if nd == 1:
            pos = pos[..., 0].contiguous()  # (B, L): the reference unsqueezes it (enc_grid.py:43-44)
        sc = (rnd(B, pde.n_cond_spatial, *spatial, lo=0.0, hi=1.0) > 0.8).float() if pde.n_cond_spatial else None
        y = m(x, cond=cond, bc=None, pos=pos, t_cond=None, spatial_cond=sc)
        assert y.shape == x.shape
        g = rnd(*y.shape)
        y.backward(g)
        grads = {k: v.grad.clone() for k, v in m.named_parameters()}
        assert all(v is not None and v.abs().max() > 0 for v in grads.values())
        rec = dict(kwargs={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, pde=dict(case["pde"]),
                   state_dict={k: v.detach().clone() for k, v in m.state_dict().items()}, x=x, cond=cond, pos=pos,
                   y=y.detach().clone(), g=g)
        if sc is not None:
            rec["spatial_cond"] = sc
        if name == "epd3d_fno":
            big[name] = grads
        else:
            rec["grads"] = grads
        out[name] = rec

    for fname, payload in (("encprocdec_nd.pt", out), ("encprocdec_nd_grads3d.pt", big)):
        path = os.path.join(HERE, fname)
        torch.save(payload, path)
        size = os.path.getsize(path)
        assert size < (1 << 20), (fname, size)
        print(f"wrote {fname}  ({size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
