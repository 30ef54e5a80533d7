"""Generate the U-Net attention fixtures (tests/golden/attention.pt: cases a-c, attention_model.pt: case d)
from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (mounted read-only at
/root/reference) and stores plain tensors only — seeded state_dicts, inputs, outputs and the reference's own
autograd gradients.  Nothing on the GPU box or in the product path runs it.

Cases (reference proc_unet_modern.py:253-317 AttentionBlock, :24-196 UNetModern):
  a  AttentionBlock(16) on (2, 16, 7, 9): identity shortcut, one head, d_k = channels
  b  AttentionBlock(8, out_channels=16, n_heads=2, d_k=12) on (2, 8, 5, 6): two heads and the kernel-1 shortcut
     conv.  The reference's forward cannot run this block: with more than one head `res.view` (:308) meets a
     non-contiguous einsum result, and the shortcut conv is handed the token-major [B, N, C] view (:313).  The
     fixture is therefore the reference's own modules and parameters evaluated line by line with the two
     evident repairs — `reshape` for that `view`, and the shortcut applied channel-major, conv(x.view(B, C, N)),
     then moved to token-major — recorded in the fixture as `restated=True`.
  c  UNetModern(hidden 8, n_cond 2, ch_mults [1, 2], is_attn [False, True], mid_attn, norm) at 32 x 32, B = 2
  d  the same U-Net inside one tiny full EncProcDec model (one model call)

Usage (from any cwd):  python tests/golden/make_golden_attn.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_stubs, REF_SRC  # noqa: E402


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    from torch import nn
    torch.set_num_threads(8)
    import models
    from models.enc_proc_dec_components import proc_unet_modern as pum
    from pdes import PDE2D

    gen = torch.Generator().manual_seed(4321)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    out = {}

    def grads(m):
        return {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()}

    # ---- (a), (b): AttentionBlock with gradients ----
    def block_case(name, kw, xs, restated):
        torch.manual_seed(42)
        m = pum.AttentionBlock(**kw)
        x = rnd(*xs).requires_grad_(True)
        if restated:
            B = xs[0]
            tok = x.view(B, m.in_channels, -1).permute(0, 2, 1)
            qkv = m.projection(tok).view(B, -1, m.n_heads, 3 * m.d_k)
            q, k, v = torch.chunk(qkv, 3, dim=-1)
            attn = (torch.einsum("bihd,bjhd->bijh", q, k) * m.scale).softmax(dim=1)
            res = torch.einsum("bijh,bjhd->bihd", attn, v).reshape(B, -1, m.n_heads * m.d_k)
            res = m.output(res) + m.shortcut(x.view(B, m.in_channels, -1)).permute(0, 2, 1)
            y = res.permute(0, 2, 1).reshape(B, m.out_channels, *xs[2:])
        else:
            y = m(x)
        g = rnd(*y.shape)
        y.backward(g)
        out[name] = dict(kwargs=kw, state_dict={k: v.clone() for k, v in m.state_dict().items()}, x=x.detach().clone(),
                         y=y.detach().clone(), g=g, dx=x.grad.clone(), grads=grads(m),
                         restated=restated)

    block_case("a", dict(in_channels=16), (2, 16, 7, 9), False)
    block_case("b", dict(in_channels=8, out_channels=16, n_heads=2, d_k=12), (2, 8, 5, 6), True)

    # ---- (c): U-Net with attention in the second level, the middle and the matching up blocks ----
    gelu = nn.GELU()
    ukw = dict(num_spatial_dims=2, n_cond=2, hidden_features=8, activation=gelu, norm=True, ch_mults=[1, 2],
               is_attn=[False, True], mid_attn=True, n_blocks=1, use1x1=True, padding_mode="circular")
    torch.manual_seed(42)
    m = pum.UNetModern(pde=None, **ukw)
    h = rnd(2, 8, 32, 32).requires_grad_(True)
    vb = rnd(2, 2, 32, 32, lo=0.0, hi=1.0)
    y = m(h=h, variables_broadcast=vb, pos=None)
    g = rnd(*y.shape)
    y.backward(g)
    out["c"] = dict(kwargs={k: v for k, v in ukw.items() if k != "activation"},
                    state_dict={k: v.clone() for k, v in m.state_dict().items()}, h=h.detach().clone(), vb=vb,
                    y=y.detach().clone(), g=g, dh=h.grad.clone(), grads=grads(m))

    # ---- (d): one call of a full model around that U-Net (as model_unet in make_golden.py) ----
    res = 16
    cfg = dict(activation_final=nn.Tanh(), enforce_spatial_cond=True, spatial_cond_channel=0,
               approx_volume_preserve=True, approx_volume_preserve_mode="individual_static", max_pct_dif=1 / 25,
               model_class="EncProcDec", num_spatial_dims=2, time_window=25, data_structure="grid",
               processor_residual=False, encoder="enc_grid.ElementWise", activation=gelu,
               decoder="dec_grid.TimeConvDense", dec_delta_mode="per_step",
               num_c=1, processor="UNetModern", ch_mults=[1, 2], is_attn=[False, True], mid_attn=True,
               hidden_features=8, norm=True, use1x1=True, cond_mode="concat", padding_mode="circular",
               dec_kernel_size=5, dec_padding_mode="circular")
    torch.manual_seed(42)
    pde = PDE2D(tmin=0.0, tmax=1.0, nt=501, L1=1.0, L2=1.0, nx1=res, nx2=res, x=None, name="twophase",
                n_cond_static=3, n_cond_spatial=1)
    model = models.activation_wrapper(**cfg, pde=pde)
    model.eval()
    B, tw = 2, 25
    xs = torch.linspace(0, 1, res)
    X, Y = torch.meshgrid(xs, xs, indexing="ij")
    ts = torch.linspace(0, 1, tw)
    phase = torch.rand(B, 1, 1, 1, 1, generator=gen) * 6.28
    u = 0.5 + 0.5 * torch.tanh((Y[None, None, None] - 0.3 - 0.4 * ts[None, None, :, None, None]
                                - 0.1 * torch.sin(2 * 3.14159265 * X[None, None, None] + phase)) / 0.05)
    u = (u + 0.02 * torch.rand(B, 1, tw, res, res, generator=gen)).float()
    cond = torch.rand(B, 3, generator=gen)
    pos = torch.stack([X, Y], dim=-1)[None].repeat(B, 1, 1, 1)
    spatial_cond = (torch.rand(B, 1, res, res, generator=gen) > 0.9).float()
    with torch.no_grad():
        y = model(u, cond=cond, bc=None, pos=pos, t_cond=None, spatial_cond=spatial_cond)
    model_case = dict(cfg={k: v for k, v in cfg.items() if k not in ("activation", "activation_final")},
                    pde=dict(tmin=0.0, tmax=1.0, nt=501, nx1=res, nx2=res, n_cond_static=3, n_cond_spatial=1),
                    state_dict={k: v.clone() for k, v in model.state_dict().items()}, u=u, cond=cond, pos=pos,
                    spatial_cond=spatial_cond, y=y)

    # two files: together the four cases pass the repository's 1 MiB limit for a committed file
    for fname, payload in (("attention.pt", out), ("attention_model.pt", dict(d=model_case))):
        path = os.path.join(HERE, fname)
        torch.save(payload, path)
        print(f"wrote {fname}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
