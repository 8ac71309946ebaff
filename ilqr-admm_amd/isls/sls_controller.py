"""SLS controller synthesis on the device: K = PHI_U Phi_x^-1, k = (I - K Su) du for a batch of problems (isls_sls_controller).

The kernel uses that Phi_x = Sw + Su PHI_U is unit block lower triangular for a causal PHI_U: block column recursions through
the dynamics and a block back-substitution per row of K replace the dense transfer matrices and the (N n)^2 inverse of
sls_dense.controller (isls/sls.py:235-242).  It computes in fp64 whatever the solver's dtype is, as the host path does.
Problems the kernel flags as not causal, and dimensions beyond its limits (n <= 16, m <= 8), take sls_dense.controller.
"""
import numpy as np
import torch

from . import _capi as capi

WORK_CAP_BYTES = 2 << 30        # the workspace grows as B N^2 n^2 / 2: larger batches run in chunks that stay under this


def synthesize(engine, A, Bm, PHI_U, du, dense_one, work_cap_bytes=WORK_CAP_BYTES):
    """Controllers of PHI_U [N m, N n] / [B, N m, N n] and du [N m] / [B, N m], numpy or torch on the engine's device.

    A [Ba, Na, n, n], Bm [Ba, Na, n, m]: fp64 device tensors whose leading dimensions broadcast to (B, N) (Ba = 1 shares
    the dynamics over the batch, Na = 1 over the horizon).  dense_one(b, PHI_U_b, du_b) -> (K_b, k_b) is the host route for
    problem b.  Returns (K, k, flags): numpy float64 for numpy inputs, fp64 tensors on the engine's device for torch inputs;
    flags [B] (numpy int32) holds capi.CTL_NOT_CAUSAL for the problems that took the host route because of PHI_U."""
    dev = engine.device
    torch_in = isinstance(PHI_U, torch.Tensor)
    as_dev = lambda x: (x.to(device=dev, dtype=torch.float64) if isinstance(x, torch.Tensor)           # noqa: E731
                        else torch.as_tensor(np.asarray(x, dtype=np.float64), device=dev)).contiguous()
    P, d = as_dev(PHI_U), as_dev(du)
    single = P.ndim == 2
    if single:
        P = P[None]
    if d.ndim == 1:
        d = d[None].expand(P.shape[0], -1).contiguous()
    B, R, Cn = P.shape
    n, m = Bm.shape[-2], Bm.shape[-1]
    N = R // m
    if R != N * m or Cn != N * n or tuple(d.shape) != (B, R):
        raise ValueError(f"PHI_U {tuple(P.shape)} / du {tuple(d.shape)} do not match x_dim={n}, u_dim={m}")
    K = torch.empty_like(P)
    k = torch.empty_like(d)
    flags = np.zeros(B, dtype=np.int32)
    if n <= 16 and m <= 8:
        fl = torch.empty(B, dtype=torch.int32, device=dev)
        per = capi.sls_controller_work_elems(1, N, n)
        chunk = max(1, min(B, int(work_cap_bytes) // (8 * per)))
        work = torch.empty(chunk * per, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            pick = lambda x: x if x.shape[0] == 1 else x[b0:b1]                                         # noqa: E731
            engine.kern.sls_controller(pick(A), pick(Bm), P[b0:b1], d[b0:b1], K[b0:b1], k[b0:b1], fl[b0:b1], work,
                                       stream=stream)
        flags = fl.cpu().numpy()
        host = np.flatnonzero(flags)
    else:
        host = np.arange(B)
    for b in host:                                              # not causal, or beyond the kernel's dimensions
        Kb, kb = dense_one(int(b), P[b].cpu().numpy(), d[b].cpu().numpy())
        K[b].copy_(torch.as_tensor(Kb, device=dev))
        k[b].copy_(torch.as_tensor(kb, device=dev))
    if single:
        K, k = K[0], k[0]
    if not torch_in:
        K, k = K.cpu().numpy(), k.cpu().numpy()
    return K, k, flags
