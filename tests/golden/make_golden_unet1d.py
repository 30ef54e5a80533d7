"""Generate the 1-D U-Net / U-FNO fixtures (tests/golden/unet1d_*.pt) from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (make_golden.REF_SRC) and stores plain
tensors only.  Nothing on the GPU box or in the product path runs it.

Every case builds the reference's real module under torch.manual_seed(42), runs it in fp32 and, from a copy cast to
float64 (the FNO's complex parameters to complex128 by hand: .double() leaves them complex64), in fp64, each under the
same random cotangent g.  Stored per case, in unet1d_<case>.pt:
  kind / kwargs (/ pde), state_dict (fp32), the inputs, g,
  y64       the fp64 output,
  e_ref     {"y": rel-L2 of the reference's own fp32 output against y64, parameter name: the same for its gradient}
  blocks    (the first U-Net case only) {submodule name: dict(inputs=(fp32 tensors the fp32 run fed it), out64=the fp64
            submodule's outputs on exactly those inputs)} for a ResidualBlock with a 1x1 shortcut, one with the
            identity shortcut, the Downsample with conditioning and the Upsample
and in unet1d_<case>_grads.pt: {parameter name: fp64 gradient}; parameters the reference leaves without a gradient
(the attention block's unused norm) are absent there.

Cases (module level: (B, C, L) inputs with variables_broadcast (B, n_cond, L)):
  unet_l13      UNetModern(num_spatial_dims=1, n_cond=2, hidden_features=16, ch_mults=(1, 2), n_blocks=1, norm=True,
                is_attn=(False, True), mid_attn=True, padding_mode="ones", use1x1=False) at L = 13 (13 -> 7 -> 14: the
                skip is padded into the up frame, the output cropped)
  unet_l64      the same U-Net at L = 64
  unet_plain    norm=False, use1x1=True, no attention, n_cond=0, one level of two blocks (ch_mults=(1,), n_blocks=2)
                at L = 20.  One level because the reference cannot run n_cond=0 through a Downsample: without
                variables_broadcast its Downsample returns a bare tensor that the U-Net unpacks along the batch, and
                its up path crops variables_broadcast unconditionally; it is given a zero-channel (B, 0, L)
                variables_broadcast here, which no Downsample has to convolve.
  unet_nonorm   norm=False, use1x1=True, no attention, n_cond=2, two levels, at L = 20 (the plain route through the
                Downsample and the Upsample)
  ufno_l37      UFNO(num_spatial_dims=1, n_cond=2, hidden_features=16, hidden_blocks=2, fno_modes=5, norm=True,
                padding_mode="ones") at L = 37
  epd_unet_l37  EncProcDec(ElementWise / TimeConvDense, num_c=2, time_window=5, stub dt=0.5, n_cond_static=2) around
                that UNetModern (without attention) at L = 37
  epd_ufno_l72  the same around that UFNO at L = 72

Usage (from any cwd):  python tests/golden/make_golden_unet1d.py
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

UNET = dict(num_spatial_dims=1, n_cond=2, hidden_features=16, ch_mults=[1, 2], n_blocks=1, norm=True,
            is_attn=[False, True], mid_attn=True, padding_mode="ones", use1x1=False)
UNET_PLAIN = dict(num_spatial_dims=1, n_cond=0, hidden_features=16, ch_mults=[1], n_blocks=2, norm=False,
                  is_attn=[False], mid_attn=False, padding_mode="ones", use1x1=True)
UNET_NONORM = dict(num_spatial_dims=1, n_cond=2, hidden_features=16, ch_mults=[1, 2], n_blocks=1, norm=False,
                   is_attn=[False, False], mid_attn=False, padding_mode="ones", use1x1=True)
UFNO = dict(num_spatial_dims=1, n_cond=2, hidden_features=16, hidden_blocks=2, fno_modes=5, norm=True,
            padding_mode="ones", cond_mode="concat")
EPD = dict(encoder="enc_grid.ElementWise", decoder="dec_grid.TimeConvDense", num_spatial_dims=1, num_c=2,
           time_window=5, hidden_features=16, cond_mode="concat")
PDE = dict(dt=0.5, n_cond_static=2, n_cond_spatial=0)
CASES = {
    "unet_l13": dict(kind="UNetModern", kwargs=UNET, L=13, blocks=["down.0.res", "middle.res2", "down.1", "up.2"]),
    "unet_l64": dict(kind="UNetModern", kwargs=UNET, L=64),
    "unet_plain": dict(kind="UNetModern", kwargs=UNET_PLAIN, L=20),
    "unet_nonorm": dict(kind="UNetModern", kwargs=UNET_NONORM, L=20),
    "ufno_l37": dict(kind="UFNO", kwargs=UFNO, L=37),
    "epd_unet_l37": dict(kind="EncProcDec", kwargs=dict(EPD, processor="UNetModern", ch_mults=[1, 2], n_blocks=1,
                                                        norm=True, padding_mode="ones", use1x1=False), L=37),
    "epd_ufno_l72": dict(kind="EncProcDec", kwargs=dict(EPD, processor="UFNO", hidden_blocks=2, fno_modes=5, norm=True,
                                                        padding_mode="ones"), L=72),
}
B = 2


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    from torch import nn
    torch.set_num_threads(8)
    from models.enc_proc_dec import EncProcDec
    from models.enc_proc_dec_components.proc_unet_modern import UNetModern
    from models.enc_proc_dec_components.proc_ufno import UFNO as RefUFNO

    gen = torch.Generator().manual_seed(1618)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    def to64(m):
        m64 = copy.deepcopy(m).double()
        for p in m64.parameters():
            if p.is_complex():
                p.data = p.data.to(torch.complex128)
        return m64

    def dbl(t):
        return None if t is None else t.double()

    def rel(a, b):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        return (torch.linalg.vector_norm(a.double() - b.double()) / torch.linalg.vector_norm(b.double())).item()

    for name, case in CASES.items():
        kw, L, kind = case["kwargs"], case["L"], case["kind"]
        torch.manual_seed(42)
        if kind == "EncProcDec":
            m = EncProcDec(pde=types.SimpleNamespace(**PDE), activation=nn.GELU(), **kw)
            x = rnd(B, kw["num_c"], kw["time_window"], L, lo=0.0, hi=1.0)
            cond = rnd(B, PDE["n_cond_static"], lo=0.0, hi=1.0)
            pos = torch.linspace(0, 1, L)[None].repeat(B, 1).contiguous()
            inputs = dict(x=x, cond=cond, pos=pos)
            call = lambda mod, c: mod(c(x), cond=c(cond), bc=None, pos=c(pos), t_cond=None, spatial_cond=None)  # noqa: E731
        else:
            cls = UNetModern if kind == "UNetModern" else RefUFNO
            m = cls(pde=None, activation=nn.GELU(), **kw)
            x = rnd(B, kw["hidden_features"], L)
            vb = rnd(B, kw["n_cond"], L) if kw["n_cond"] else None
            inputs = dict(x=x, vb=vb)
            vb_ref = vb if vb is not None else torch.zeros(B, 0, L)  # (the reference's up path always crops it)
            call = lambda mod, c: mod(c(x), variables_broadcast=c(vb_ref))  # noqa: E731
        # the fp32 run, with the inputs of the recorded submodules
        seen = {}
        hooks = [m.get_submodule(b).register_forward_hook(
            lambda mod, args, out, b=b: seen.__setitem__(b, tuple(a.detach().clone() for a in args)))
            for b in case.get("blocks", [])]
        y32 = call(m, lambda t: t)
        for h in hooks:
            h.remove()
        g = rnd(*y32.shape)
        y32.backward(g)
        m64 = to64(m)
        y64 = call(m64, dbl)
        y64.backward(g.double())
        g32 = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        g64 = {k: p.grad.detach().clone() for k, p in m64.named_parameters() if p.grad is not None}
        assert set(g32) == set(g64) and all(v.abs().max() > 0 for v in g64.values())
        e_ref = {k: rel(g32[k], g64[k]) for k in g64}
        e_ref["y"] = rel(y32.detach(), y64.detach())
        rec = dict(kind=kind, kwargs=dict(kw), state_dict={k: v.detach().clone() for k, v in m.state_dict().items()},
                   g=g, y64=y64.detach().clone(), e_ref=e_ref, **{k: v for k, v in inputs.items() if v is not None})
        if kind == "EncProcDec":
            rec["pde"] = dict(PDE)
        if seen:
            blocks = {}
            for b, args in seen.items():
                with torch.no_grad():
                    out = m64.get_submodule(b)(*[a.double() for a in args])
                out = out if isinstance(out, tuple) else (out,)
                blocks[b] = dict(inputs=args, out64=tuple(o.detach().clone() for o in out))
            rec["blocks"] = blocks
        gs = sorted(v for k, v in e_ref.items() if k != "y")
        print(f"{name}: y e_ref {e_ref['y']:.2e}; gradients e_ref median {gs[len(gs) // 2]:.2e} worst {gs[-1]:.2e} "
              f"({len(g64)} with a gradient of {len(list(m.parameters()))} parameters)")
        for fname, payload in ((f"unet1d_{name}.pt", rec), (f"unet1d_{name}_grads.pt", g64)):
            path = os.path.join(HERE, fname)
            torch.save(payload, path)
            size = os.path.getsize(path)
            assert size < (1 << 20), (fname, size)
            print(f"  wrote {fname}  ({size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
