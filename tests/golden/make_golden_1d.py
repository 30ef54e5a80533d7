"""Generate the 1-D FNO fixture (tests/golden/fno1d.pt) from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (make_golden.REF_SRC) and stores plain
tensors only — seeded state_dicts, inputs, outputs and the reference's own
autograd gradients.  Nothing on the GPU box or in the product path runs it.

Cases (reference proc_fno.py:158-222 SpectralConv1d, :87-155 FNO_Layer, :22-83 FNO), each constructed under
torch.manual_seed(42) with feature_transform_dim = 3 and p ~ U[0, 1):
  spectral1d_a 6 -> 5, m = 4 on (2, 6, 16); spectral1d_nyq 3 -> 2, m = 5 on (1, 3, 8) (m == L//2+1, even L);
      spectral1d_odd 3 -> 4, m = 4 on (2, 3, 7) (m == L//2+1, odd L) — each without FiLM ("<name>") and with
      transform_mode 0 and 1 ("<name>_tm<mode>")
  fno_layer1d: FNO_Layer 6 -> 5, modes 4, GELU, FiLM (transform_mode 0, the layer's default) on (2, 6, 16)
  fno_layer1d_double: the same with conv_mode="double", kernel_size=1, no FiLM
  fno1d_film: FNO(num_spatial_dims=1, n_cond=3, hidden_features=8, fno_modes=3, hidden_blocks=2, cond_mode="film")
      on (2, 8, 16), called as forward(h, variables=p)
  fno1d_concat: the same with n_cond=2, cond_mode="concat" and variables_broadcast vb (2, 2, 16)
Every case records kwargs, state_dict, x, (p | vb), y, g, dx, (dp | dvb) and the gradient of every parameter.

Usage (from any cwd):  python tests/golden/make_golden_1d.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_stubs, REF_SRC  # noqa: E402

SPECTRAL_CASES = [
    ("spectral1d_a", dict(in_channels=6, out_channels=5, modes=(4,)), (2, 6, 16)),
    ("spectral1d_nyq", dict(in_channels=3, out_channels=2, modes=(5,)), (1, 3, 8)),
    ("spectral1d_odd", dict(in_channels=3, out_channels=4, modes=(4,)), (2, 3, 7)),
]
K = 3


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    torch.set_num_threads(8)
    from models.enc_proc_dec_components.proc_fno import SpectralConv1d, FNO_Layer, FNO

    gen = torch.Generator().manual_seed(1618)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    out = {}

    def record(name, m, kwargs, xs, call, p_shape=None, vb_shape=None):
        x = rnd(*xs).requires_grad_(True)
        p = rnd(*p_shape, lo=0.0, hi=1.0).requires_grad_(True) if p_shape else None
        vb = rnd(*vb_shape).requires_grad_(True) if vb_shape else None
        y = call(m, x, p, vb)
        g = rnd(*y.shape)
        y.backward(g)
        rec = dict(kwargs=kwargs, state_dict={k: v.detach().clone() for k, v in m.state_dict().items()},
                   x=x.detach().clone(), y=y.detach().clone(), g=g, dx=x.grad.clone(),
                   grads={k: v.grad.clone() for k, v in m.named_parameters()})
        if p is not None:
            rec.update(p=p.detach().clone(), dp=p.grad.clone())
        if vb is not None:
            rec.update(vb=vb.detach().clone(), dvb=vb.grad.clone())
        out[name] = rec

    for name, kw, xs in SPECTRAL_CASES:
        torch.manual_seed(42)
        m = SpectralConv1d(**kw)
        record(name, m, dict(kw, modes=list(kw["modes"])), xs, lambda m, x, p, vb: m(x))
        for tm in (0, 1):
            full = dict(kw, feature_transform=True, feature_transform_dim=K, transform_mode=tm)
            torch.manual_seed(42)
            m = SpectralConv1d(**full)
            record(f"{name}_tm{tm}", m, dict(full, modes=list(kw["modes"])), xs, lambda m, x, p, vb: m(x, p),
                   p_shape=(xs[0], K))

    kw = dict(hidden_dim=6, num_spatial_dims=1, modes=4, hidden_dim_out=5, feature_transform=True,
              feature_transform_dim=K, padding_mode="circular")
    torch.manual_seed(42)
    m = FNO_Layer(**kw)
    record("fno_layer1d", m, kw, (2, 6, 16), lambda m, x, p, vb: m(x, p), p_shape=(2, K))

    kw = dict(hidden_dim=6, num_spatial_dims=1, modes=4, hidden_dim_out=5, conv_mode="double", kernel_size=1,
              padding_mode="circular")
    torch.manual_seed(42)
    m = FNO_Layer(**kw)
    record("fno_layer1d_double", m, kw, (2, 6, 16), lambda m, x, p, vb: m(x))

    kw = dict(num_spatial_dims=1, n_cond=K, hidden_features=8, fno_modes=3, hidden_blocks=2, cond_mode="film")
    torch.manual_seed(42)
    m = FNO(pde=None, **kw)
    record("fno1d_film", m, kw, (2, 8, 16), lambda m, x, p, vb: m(x, variables=p), p_shape=(2, K))

    kw = dict(num_spatial_dims=1, n_cond=2, hidden_features=8, fno_modes=3, hidden_blocks=2, cond_mode="concat")
    torch.manual_seed(42)
    m = FNO(pde=None, **kw)
    record("fno1d_concat", m, kw, (2, 8, 16), lambda m, x, p, vb: m(x, variables_broadcast=vb), vb_shape=(2, 2, 16))

    path = os.path.join(HERE, "fno1d.pt")
    torch.save(out, path)
    print(f"wrote fno1d.pt  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
