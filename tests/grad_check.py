"""The parameter-gradient check shared by the GPU backward tests."""
import torch

TOL = 1e-5  # the fp32 bar (BASELINE.json north star)


def grads_ok(named_ref, named_got, tol=TOL, tensor_tol=1e-4):
    """All parameter gradients as one vector: rel-L2 < tol (1e-5).  Per tensor: rel-L2 < tensor_tol, or an
    error below tol x the norm of the whole gradient — bias / GroupNorm-affine gradients are sums over every
    pixel that largely cancel (fp32 noise of such a sum is ~eps x the cancellation factor, on the CPU
    reference as much as here), and a bias feeding a per-channel GroupNorm (e.g. the last UpBlock's
    shortcut bias before GroupNorm(8, 8)) has an analytically zero gradient that both sides only resolve
    to rounding noise."""
    keys = list(named_ref)
    for k in keys:
        assert named_got[k] is not None, f"no gradient for {k}"
    ref = torch.cat([torch.view_as_real(named_ref[k]).reshape(-1) if named_ref[k].is_complex()
                     else named_ref[k].reshape(-1) for k in keys]).double()
    got = torch.cat([(torch.view_as_real(named_got[k]) if named_got[k].is_complex() else named_got[k])
                     .reshape(-1).cpu() for k in keys]).double()
    e_all = (torch.linalg.vector_norm(got - ref) / torch.linalg.vector_norm(ref)).item()
    total = torch.linalg.vector_norm(ref).item()
    bad = []
    for k in keys:
        r = named_ref[k].detach().cpu()
        g = named_got[k].detach().cpu()
        if r.is_complex():
            r, g = torch.view_as_real(r), torch.view_as_real(g)
        r, g = r.double(), g.double()
        d = torch.linalg.vector_norm(g - r).item()
        e = d / max(torch.linalg.vector_norm(r).item(), 1e-30)
        if not (e < tensor_tol or d < tol * total):
            bad.append((k, e, d / total))
    assert e_all < tol and not bad, (e_all, bad)
