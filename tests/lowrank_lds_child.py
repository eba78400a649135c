"""Child process of tests/test_gpu_lowrank.py::test_dynamic_lds_opt_in_survives_a_larger_second_model: in a process where nothing has launched
yet, the low-rank entry points whose dynamic LDS grows with the model are called with a small model first and a large one second (`both`), or
with the large one alone (`large`).  The opt-in for dynamic LDS above 48 KB is set once per kernel and device (csrc/jf_common.h: LdsAttrOnce),
so the size it is set to must not be the first call's.  Writes what the large calls returned to the .npz file named on the command line.

Shapes, from the size formulas in csrc/amlp_gf_kernels.hip (float64, 8 bytes; the opt-in is needed above 48 KB = 49152 bytes, a workgroup may
take 160 KB = 163840 bytes):

  jf_lowrank_head_bwd_f64 (lrm_bwd_lds), doubles = (H/16) 128 + (H/4) 64 + KT 128 + psz + 2176 with KT = ceil(K1 / 16), psz = 17 H + 128 KT;
  lrm_shape_ok admits H = 16, 32 .. 128 and K1 <= 32, one kernel instance for KT = 1 and one for KT = 2:
    H =  16, KT = 1:  128 +  256 + 128 +  400 + 2176 = 3088 doubles = 24704 bytes   (smallest H)
    H = 128, KT = 1: 1024 + 2048 + 128 + 2304 + 2176 = 7680 doubles = 61440 bytes   (largest H admitted: every admitted shape is <= 160 KB)
    H =  16, KT = 2:  128 +  256 + 256 +  528 + 2176 = 3344 doubles = 26752 bytes
    H = 128, KT = 2: 1024 + 2048 + 256 + 2432 + 2176 = 7936 doubles = 63488 bytes   (the largest of all admitted shapes)
  jf_lowrank_gf_chain_inv_f64, doubles = n_layers (21 * 128 + 21 * 16) = 3024 n_layers, 24192 bytes per layer:
    n_layers = 2:  48384 bytes (no opt-in yet)      n_layers = 3:  72576 bytes (smallest above 48 KB)
    n_layers = 6: 145152 bytes (largest <= 160 KB)  n_layers = 7: 169344, n_layers = 8 = JF_MAX_CHAIN: 193536 bytes -> refused as unsupported
"""
import sys

import numpy as np
import torch

import jammy_flows_amd
from jammy_flows_amd import _hip
from jammy_flows_amd.amortizable_mlp import AmortizableMLP

B, D = 33, 2
HEAD_SMALL = {1: (6, 16, 2, 2, 8), 2: (17, 16, 2, 2, 8)}          # KT -> (K1, H, r1, r2, N)
HEAD_LARGE = {1: (16, 128, 8, 8, 16), 2: (32, 128, 8, 8, 16)}
CHAIN_SMALL, CHAIN_LARGE, CHAIN_TOO_LONG = 3, 6, 8


def head(shape, out, key):
    """_hip.lowrank_head / _hip.lowrank_head_bwd on the weights of an AmortizableMLP, and the same quantities from the module's per-stage launches
    (head_one_launch = False: the reference of test_lowrank_head_equals_the_stage_sequence)"""
    K1, H, r1, r2, N = shape
    torch.manual_seed(K1 * 1000 + H)
    mlp = AmortizableMLP(K1, str(H), N, low_rank_approximations=[r1, r2], use_permanent_parameters=True).double().cuda()
    with torch.no_grad():
        mlp.u_v_b_pars.add_(0.2 * torch.randn_like(mlp.u_v_b_pars))
    assert not mlp.stages[0]["full"] and not mlp.stages[1]["full"]
    x = torch.randn(B, K1, dtype=torch.float64, device="cuda")
    w = torch.randn(B, N, dtype=torch.float64, device="cuda")
    v1, u1, b1, v2, u2, b2 = mlp.lowrank_views(mlp.u_v_b_pars.detach().reshape(-1))
    t2, t1, h = _hip.lowrank_head(x, v1, u1, b1, v2)
    got = _hip.lowrank_head_bwd(x, v1, u1, v2, t1, h, w @ u2, True)
    torch.cuda.synchronize()
    if out is None:
        return
    mlp.head_one_launch = False
    xs = x.clone().requires_grad_(True)
    timer = _hip.KernelTimer()
    with torch.enable_grad(), timer:
        ref_out = mlp(xs)
        (ref_out * w).sum().backward()
    assert not any("lowrank_head" in k[0] for k in timer.summary())
    r_v1, r_u1, r_b1, r_v2, _, _ = mlp.lowrank_views(mlp.u_v_b_pars.grad.reshape(-1))
    for name, t in (("t2", t2), ("t1", t1[:, :r1]), ("h", h), ("out", t2 @ u2.t() + b2), ("ref_out", ref_out.detach())):
        out["%s.%s" % (key, name)] = t.cpu().numpy()
    for name, g, r in zip(("g_inp", "g_v1", "g_u1", "g_b1", "g_v2"), got, (xs.grad, r_v1, r_u1, r_b1, r_v2)):
        out["%s.%s" % (key, name)] = g.cpu().numpy()
        out["%s.ref_%s" % (key, name)] = r.cpu().numpy()
    out[key + ".ref_par_absmax"] = mlp.u_v_b_pars.grad.abs().max().cpu().numpy()      # the scale of that test's bound on the weight gradients


def chain(layers, n_layers, out, key):
    larr = _hip.gf_layer_array([l.c_struct() for l in layers[:n_layers]])
    N = sum(l.total_param_num for l in layers[:n_layers])
    g = torch.Generator(device="cuda").manual_seed(3 + n_layers)
    t2 = torch.randn(B, 8, dtype=torch.float64, device="cuda", generator=g)
    u2 = torch.randn(N, 8, dtype=torch.float64, device="cuda", generator=g) * 0.2
    b2 = torch.randn(N, dtype=torch.float64, device="cuda", generator=g) * 0.5
    x = torch.randn(B, D, dtype=torch.float64, device="cuda", generator=g)
    ld = torch.randn(B, dtype=torch.float64, device="cuda", generator=g)
    res = _hip.lowrank_gf_chain_inv(t2, u2, b2, x, ld, larr, n_layers, D, want_base_logp=True)
    torch.cuda.synchronize()
    if out is None:
        return
    out[key + ".supported"] = np.array(res is not None)
    if res is not None:
        for name, t in zip(("z", "ld", "blp"), res):
            out["%s.%s" % (key, name)] = t.cpu().numpy()


def main():
    mode, path = sys.argv[1], sys.argv[2]
    assert mode in ("both", "large")
    torch.manual_seed(0)
    pdf = jammy_flows_amd.pdf("e%d" % D, "g" * CHAIN_TOO_LONG, conditional_input_dim=6, amortization_mlp_use_custom_mode=True,
                              amortization_mlp_dims="64", amortization_mlp_ranks=8).double().cuda()
    layers = list(pdf.layer_list[0])
    out = {}
    for kt in (1, 2):
        if mode == "both":
            head(HEAD_SMALL[kt], None, None)
        head(HEAD_LARGE[kt], out, "head%d" % kt)
    if mode == "both":
        chain(layers, CHAIN_SMALL, None, None)
    chain(layers, CHAIN_LARGE, out, "chain")
    chain(layers, CHAIN_TOO_LONG, out, "chain_max")
    np.savez(path, **out)
    print("lowrank_lds_child %s: %d arrays" % (mode, len(out)))


if __name__ == "__main__":
    main()
