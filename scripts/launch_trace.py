"""Launch trace of pdf's block loops: which kernels a call launches, in which order, and the bits it returns.

For every top-level fixture of tests/golden that the library can build, in float32 and float64, a fixed list of calls through the public API
(pdf(...), planned_forward, sample, entropy) is run under _hip.KernelTimer.  Each case becomes one JSON line

    {"case": id, "launches": [[name, tag], ...], "sha256": digest of the bytes of every returned tensor,
     "sha256_grads": the same of every gradient (gradient cases)}

(planned calls: the names in plan.calls and plan.n_ops).  Two checkouts that choose and sequence the launches alike write identical files;
run it at both and diff.  Values from kernels with floating-point atomics (some gradients) may differ from run to run of ONE checkout:
run twice at the older checkout and compare such cases on their launch lists alone.

    python scripts/launch_trace.py --out trace.jsonl [--repo /path/to/checkout] [--only c3_e4s2e4]

A case that raises is recorded with the exception's type and text in place of the digest.  The process ends with a non-zero status on the
first device-side failure.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROWS = 257                      # not a multiple of any tile
ROWS_LARGE = 4173
SCHEDULED = ["c3_e4s2e4", "c5_e8s2_ggggv", "c4_i1s1_ro", "g_e1e2e1_cond_lowrank", "mix_e2s1i1"]
VARIANTS = [("merge0", {"merge_max_rows": 0}), ("nofold", {"fold_combine": False}), ("lanes3", {"plan_lanes": 3}),
            ("overlap", {"plan_overlap_blocks": True}), ("fusedm", {"force_fused_manifold_blocks": True}),
            ("arith_f32", {"fused_matrix_arithmetic": "f32"}), ("arith_split", {"fused_matrix_arithmetic": "split"}),
            ("arith_split_f16", {"fused_matrix_arithmetic": "split_f16"}), ("nofuse", {"fuse_conditional_blocks": False})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", default=None, help="comma-separated fixture names")
    args = ap.parse_args()
    for p in (os.path.join(args.repo, "tests", "golden"), os.path.join(args.repo, "tests"), args.repo):
        sys.path.insert(0, p)
    import torch
    import fixture_io
    import helpers
    from jammy_flows_amd import _hip

    dev = "cuda:0"

    def flat(obj):
        if isinstance(obj, dict):
            return [t for k in sorted(obj, key=str) for t in flat(obj[k])]
        if isinstance(obj, (list, tuple)):
            return [t for o in obj for t in flat(o)]
        return [obj]

    def digest(obj):
        h = hashlib.sha256()
        for t in flat(obj):
            if isinstance(t, torch.Tensor):
                a = t.detach().cpu().contiguous().numpy()
                h.update(("%s%s" % (a.dtype, a.shape)).encode())
                h.update(a.tobytes())
            else:
                h.update(repr(t).encode())
        return h.hexdigest()

    out = open(args.out, "w")
    counts = {"cases": 0, "raised": 0}

    def case(cid, fn, planned=False, with_grads=False):
        """fn() -> what to hash (planned: (PlannedForward, what to hash); with_grads: (what was returned, the gradients))"""
        timer = _hip.KernelTimer()
        line = {"case": cid}
        try:
            with timer:
                res = fn()
            torch.cuda.synchronize()
            if planned:
                pf, res = res
                line["launches"] = [[c[0], c[1]] for c in pf.plan.calls]
                line["n_ops"] = pf.plan.n_ops
            else:
                line["launches"] = [[r[0], r[1]] for r in timer.records]
            if with_grads:
                res, line["sha256_grads"] = res[0], digest(res[1])
            line["sha256"] = digest(res)
        except Exception as e:      # noqa: BLE001 -- a configuration the library declines: recorded, the same at both checkouts
            line["launches"] = [[r[0], r[1]] for r in timer.records]
            line["raised"] = "%s: %s" % (type(e).__name__, str(e)[:160])
            counts["raised"] += 1
            torch.cuda.synchronize()            # a device-side failure surfaces here and ends the run
        counts["cases"] += 1
        out.write(json.dumps(line, default=str) + "\n")
        out.flush()

    def grads(pdf, leaves):
        return [p.grad for p in pdf.parameters()] + [t.grad for t in leaves if t is not None]

    def run_cases(prefix, fx, pdf, dtype, B):
        # the fixtures' rows, repeated to B rows -- without the rows that hold a column's smallest or largest value: the probes at the very
        # ends of an interval (0.999999999) leave it when rounded to float32, and a call with non-finite rows raises instead of returning
        inner = np.flatnonzero(~((fx["x"] == fx["x"].min(axis=0)) | (fx["x"] == fx["x"].max(axis=0))).any(axis=1))
        idx = inner[np.arange(B) % len(inner)]
        x = helpers.to_dev(fx["x"][idx], dtype, dev)
        cond = helpers.to_dev(None if fx.get("cond") is None else fx["cond"][idx], dtype, dev)
        with torch.no_grad():
            case(prefix + "/forward", lambda: pdf(x, conditional_input=cond))
            for coords in ("embedding", "intrinsic"):
                def forced(coords=coords):
                    xc = pdf.transform_target_space(x, transform_from="default", transform_to=coords)[0]
                    return pdf(xc, conditional_input=cond, **{"force_%s_coordinates" % coords: True})
                case(prefix + "/forward_" + coords, forced)
            case(prefix + "/forward_only_last", lambda: pdf(x, conditional_input=cond, only_last=True))

            def planned():
                pf = pdf.planned_forward(x, conditional_input=cond)
                return pf, pf(x, cond)
            case(prefix + "/planned_forward", planned, planned=True)
            case(prefix + "/sample", lambda: pdf.sample(conditional_input=cond, samplesize=B, seed=7))
            case(prefix + "/sample_embedding", lambda: pdf.sample(conditional_input=cond, samplesize=B, seed=7, force_embedding_coordinates=True))
        for streams in (1, 2):
            def train(streams=streams):
                saved = pdf.train_streams
                pdf.train_streams = streams
                try:
                    pdf.zero_grad(set_to_none=True)
                    xg = x.clone().requires_grad_(True)
                    cg = None if cond is None else cond.clone().requires_grad_(True)
                    with torch.enable_grad():
                        res = pdf(xg, conditional_input=cg)
                        res[0].sum().backward()
                    return [res, grads(pdf, [xg, cg])]
                finally:
                    pdf.train_streams = saved
            case(prefix + "/grad_streams%d" % streams, train, with_grads=True)

        def sample_grad():
            pdf.zero_grad(set_to_none=True)
            cg = None if cond is None else cond.clone().requires_grad_(True)
            with torch.enable_grad():
                res = pdf.sample(conditional_input=cg, samplesize=B, seed=7, allow_gradients=True)
                (res[0].sum() + res[2].sum()).backward()
            return [res, grads(pdf, [cg])]
        case(prefix + "/sample_grad", sample_grad, with_grads=True)
        S = 16
        c8 = None if cond is None else cond[:8].contiguous()
        torch.manual_seed(11)
        z = torch.randn((S * (1 if c8 is None else c8.shape[0]), pdf.total_base_dim), dtype=dtype, device=dev)
        subs = [-1] + list(range(len(pdf.layer_list)))
        case(prefix + "/entropy", lambda: pdf.entropy(sub_manifolds=subs, conditional_input=c8, samplesize=S, predefined_base=z))

    only = None if args.only is None else set(args.only.split(","))
    for path in fixture_io.list_fixtures():
        fx = fixture_io.Fixture(path)
        if (only is not None and fx.name not in only) or not helpers.product_supports(fx):
            continue
        for dtype, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
            pdf = helpers.build_product(fx, dtype, dev)
            run_cases("%s/%s/%d" % (fx.name, dname, ROWS), fx, pdf, dtype, ROWS)
            if fx.name in SCHEDULED:
                run_cases("%s/%s/%d" % (fx.name, dname, ROWS_LARGE), fx, pdf, dtype, ROWS_LARGE)
                for vname, attrs in VARIANTS:
                    pdf = helpers.build_product(fx, dtype, dev)
                    for k, v in attrs.items():
                        assert hasattr(pdf, k), k
                        setattr(pdf, k, v)
                    run_cases("%s/%s/%d/%s" % (fx.name, dname, ROWS, vname), fx, pdf, dtype, ROWS)
        print("%s done (%d cases, %d raised)" % (fx.name, counts["cases"], counts["raised"]), flush=True)
    out.close()
    print("launch_trace: %d cases, %d raised -> %s" % (counts["cases"], counts["raised"], args.out))


if __name__ == "__main__":
    main()
