"""Time, peak memory and mesh sizes of pdf.sky_mesh and pdf.sky_map, float32, S = 10 000 samples per conditional input:
the c3_e4s2e4 fixture (unconditional, C = 1) and the same definition behind 16 conditional inputs with its initial weights (C = 256).
sky_map runs at the order of the mesh's median finest cell where a full map of that order can be evaluated.  Medians of 5 alternating runs
in one process after a warm-up of each, a host clock around a call that ends in a device synchronise; peak memory is the allocator's peak
above what was allocated before the call.  Then the quadrature error of the mesh, |exp(log_norm) - 1| of density="model" on f_s2_cond_ff
(C = 64) for three sample sizes and both dtypes.

Needs a HIP device; it is a measurement, not a test (bench.py stays the contract benchmark)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import fixture_io  # noqa: E402
import jammy_flows_amd  # noqa: E402
from helpers import build_product, to_dev  # noqa: E402
from jammy_flows_amd import sky  # noqa: E402

F32, F64 = torch.float32, torch.float64


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return out, dt, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def mesh_stats(got):
    off = got["offsets"].cpu().numpy()
    sizes = np.diff(off)
    order = sky.order_pix_of(got["uniq"])[0]
    finest = np.array([int(order[a:b].max()) for a, b in zip(off[:-1], off[1:])])
    return sizes, finest


def run_case(title, pdf, cond, C, S, reps=5):
    print("==", title, "C =", C, "S =", S, flush=True)
    qs = (0.68, 0.9)
    mesh_fn = lambda: pdf.sky_mesh(conditional_input=cond, samplesize=S, credible_masses=qs)
    got, _, _ = timed(mesh_fn)                                # warm-up
    sizes, finest = mesh_stats(got)
    med_order = int(np.median(finest))
    print("cells per row: min %d median %d max %d total %d; finest order: min %d median %d max %d" % (
        sizes.min(), np.median(sizes), sizes.max(), sizes.sum(), finest.min(), med_order, finest.max()))
    areas = got["areas"].cpu().numpy()
    print("90 %% area: median %.4e sr; 68 %%: %.4e sr; log_norm (density = samples) max |.| %.2e" % (
        np.median(areas[:, 1]), np.median(areas[:, 0]), float(got["log_norm"].abs().max())))
    k = pdf.pdf_defs_list.index("s2")
    evals = C * (100 if k > 0 else 1) * 12 * 4 ** med_order
    map_fn = None
    if med_order <= 13 and evals <= 2e11 and C * 12 * 4 ** med_order * 4 <= 16 * 2 ** 30:
        map_fn = lambda: pdf.sky_map(med_order, conditional_input=cond, credible_masses=qs)
        m, _, _ = timed(map_fn)
        print("sky_map order %d: npix %d, 90 %% area median %.4e sr, |exp(log_norm) - 1| median %.2e" % (
            med_order, 12 * 4 ** med_order, float(m["areas"][:, 1].median()), float((m["log_norm"].exp() - 1).abs().median())))
    else:
        print("sky_map at order %d cannot run: %d pixels x %d conditional inputs (%.1e block evaluations)" % (med_order, 12 * 4 ** med_order, C, evals))
    t_mesh, m_mesh, t_map, m_map = [], [], [], []
    for _ in range(reps):                                      # alternating
        _, dt, mem = timed(mesh_fn)
        t_mesh.append(dt), m_mesh.append(mem)
        if map_fn is not None:
            _, dt, mem = timed(map_fn)
            t_map.append(dt), m_map.append(mem)
    print("sky_mesh: median %.1f ms (min %.1f max %.1f), peak memory above the model %.0f MiB" % (
        1e3 * statistics.median(t_mesh), 1e3 * min(t_mesh), 1e3 * max(t_mesh), max(m_mesh)))
    if t_map:
        print("sky_map : median %.1f ms (min %.1f max %.1f), peak memory above the model %.0f MiB" % (
            1e3 * statistics.median(t_map), 1e3 * min(t_map), 1e3 * max(t_map), max(m_map)))
    # the steps of one sky_mesh call
    dt_, dev_, _, ds = pdf._repeat_conditional(cond, S, None, None)
    (samples, _, _), t_s, _ = timed(lambda: pdf._sampling_pass(None, S * C, dt_, dev_, ds, True, False, []))
    a, b = pdf.target_dim_indices_embedded[k]
    dirs = samples[:, a:b].contiguous()
    pix, t_p, _ = timed(lambda: sky.vec2pix(29, dirs).reshape(C, S))
    mesh, t_b, _ = timed(lambda: sky.build_mesh(pix))
    print("steps: sampling %.1f ms, vec2pix(29) %.2f ms, build_mesh %.1f ms" % (1e3 * t_s, 1e3 * t_p, 1e3 * t_b), flush=True)


def main():
    torch.manual_seed(0)
    fx = fixture_io.load("c3_e4s2e4")
    run_case("C3 fixture (unconditional), float32", build_product(fx, F32), None, 1, 10000)
    # C3 behind conditional inputs: the same definition with 16 conditional inputs, weights as initialised (seed 0)
    torch.manual_seed(0)
    cpdf = jammy_flows_amd.pdf("e4+s2+e4", "gggg+f+gggg", conditional_input_dim=16).to(dtype=F32, device="cuda")
    cond = torch.randn((256, 16), generator=torch.Generator().manual_seed(1)).to("cuda")
    run_case("C3 definition with 16 conditional inputs (initial weights), float32", cpdf, cond, 256, 10000)
    # quadrature error of the mesh: density = model on an s2-first fixture
    fx = fixture_io.load("f_s2_cond_ff")
    for dtype in (F64, F32):
        pdf = build_product(fx, dtype)
        cond = to_dev(fx["cond"][:64], dtype)
        for S in (2000, 10000, 100000):
            got, dt, mem = timed(lambda: pdf.sky_mesh(conditional_input=cond, samplesize=S, credible_masses=(0.68, 0.9)))
            got, dt, mem = timed(lambda: pdf.sky_mesh(conditional_input=cond, samplesize=S, credible_masses=(0.68, 0.9)))
            sizes, finest = mesh_stats(got)
            err = (got["log_norm"].exp() - 1).abs()
            print("f_s2_cond_ff %s C = 64 S = %d: cells median %d, finest order median %d, |exp(log_norm) - 1| median %.2e max %.2e, %.1f ms, %.0f MiB" % (
                dtype, S, np.median(sizes), np.median(finest), float(err.median()), float(err.max()), 1e3 * dt, mem), flush=True)


if __name__ == "__main__":
    main()
