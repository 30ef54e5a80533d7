"""Generate the FiLM conditioning fixture (tests/golden/film.pt) from the reference implementation.

CONTAINER-ONLY TOOL, as make_golden.py: it imports the upstream reference (mounted read-only at
/root/reference) and stores plain tensors only — seeded state_dicts, inputs, outputs and the reference's own
autograd gradients.  Nothing on the GPU box or in the product path runs it.

Cases (reference proc_fno.py:225-288 SpectralConv2d with feature_transform, :87-155 FNO_Layer, :22-83 FNO), each
constructed under torch.manual_seed(42) with feature_transform_dim = 3 and p ~ U[0, 1):
  spectral2d_a / spectral2d_overlap / spectral2d_nyq, each for transform_mode 0 and 1 ("<name>_tm<mode>"): the
      kwargs and input shapes of make_golden.py's SpectralConv2d cases (overlap: 2*m1 > H, where mode 0 adds both
      corners' factors and mode 1 lets the second write win; nyq: m2 == W//2+1)
  fno_layer: FNO_Layer 6 -> 5, modes (4, 3), GELU, on (2, 6, 16, 12) (transform_mode 0, the layer's default)
  fno: FNO(cond_mode="film", n_cond=3, hidden_features=8, fno_modes=3, hidden_blocks=2) on (2, 8, 16, 12),
      called as forward(h, variables=p)
Every case records state_dict, x, p, y, g, dx, dp and the gradient of every parameter.

Usage (from any cwd):  python tests/golden/make_golden_film.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_stubs, REF_SRC  # noqa: E402

SPECTRAL_CASES = [
    ("spectral2d_a", dict(in_channels=6, out_channels=5, modes=(4, 3)), (2, 6, 16, 12)),
    ("spectral2d_overlap", dict(in_channels=3, out_channels=4, modes=(4, 3)), (2, 3, 6, 7)),
    ("spectral2d_nyq", dict(in_channels=3, out_channels=2, modes=(3, 5)), (1, 3, 8, 8)),
]
K = 3


def main():
    _install_stubs()
    os.chdir(tempfile.mkdtemp())
    sys.path.insert(0, REF_SRC)
    import torch
    torch.set_num_threads(8)
    from models.enc_proc_dec_components.proc_fno import SpectralConv2d, FNO_Layer, FNO

    gen = torch.Generator().manual_seed(2718)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return torch.rand(*shape, generator=gen) * (hi - lo) + lo

    out = {}

    def record(name, m, kwargs, xs, call):
        x = rnd(*xs).requires_grad_(True)
        p = rnd(xs[0], K, lo=0.0, hi=1.0).requires_grad_(True)
        y = call(m, x, p)
        g = rnd(*y.shape)
        y.backward(g)
        out[name] = dict(kwargs=kwargs, state_dict={k: v.detach().clone() for k, v in m.state_dict().items()},
                         x=x.detach().clone(), p=p.detach().clone(), y=y.detach().clone(), g=g, dx=x.grad.clone(),
                         dp=p.grad.clone(), grads={k: v.grad.clone() for k, v in m.named_parameters()})

    for name, kw, xs in SPECTRAL_CASES:
        for tm in (0, 1):
            full = dict(kw, feature_transform=True, feature_transform_dim=K, transform_mode=tm)
            torch.manual_seed(42)
            m = SpectralConv2d(**full)
            record(f"{name}_tm{tm}", m, dict(full, modes=list(kw["modes"])), xs, lambda m, x, p: m(x, p))

    kw = dict(hidden_dim=6, num_spatial_dims=2, modes=[4, 3], hidden_dim_out=5, feature_transform=True,
              feature_transform_dim=K, padding_mode="circular")
    torch.manual_seed(42)
    m = FNO_Layer(**dict(kw, modes=(4, 3)))
    record("fno_layer", m, kw, (2, 6, 16, 12), lambda m, x, p: m(x, p))

    kw = dict(num_spatial_dims=2, n_cond=K, hidden_features=8, fno_modes=3, hidden_blocks=2, cond_mode="film")
    torch.manual_seed(42)
    m = FNO(pde=None, **kw)
    record("fno", m, kw, (2, 8, 16, 12), lambda m, x, p: m(x, variables=p))

    path = os.path.join(HERE, "film.pt")
    torch.save(out, path)
    print(f"wrote film.pt  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
