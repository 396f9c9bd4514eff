"""float64 oracle of the Qwen3 q/k norm + RoPE, shared by
tests/test_qk_norm_ref.py and tests/test_qk_norm_gpu.py (a plain helper
module, imported the way tests/attn_boundary_cases.py is)."""

import torch


def norm_rope64(x, w, eps, pos, cos_sin):
    """float64 n = x * rsqrt(mean(x^2) + eps) * w per head and its NeoX
    half rotation; x [T, H, D].  Returns (n, rotated)."""
    xd = x.double()
    n = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    half = x.shape[-1] // 2
    cs = cos_sin.double()[pos.long()]
    c, s = cs[:, None, :half], cs[:, None, half:]
    n1, n2 = n[..., :half], n[..., half:]
    return n, torch.cat([n1 * c - n2 * s, n2 * c + n1 * s], dim=-1)
