"""--dump-outputs DIR: what the timed path returned in its last step, written as .npy files, so that two builds of the project can be compared
output for output on the same seeded inputs"""
import os

import numpy as np

DUMP_BUDGET_BYTES = 60 << 20      # all files of one run together, headers included: below 64 MB
SAMPLE_SEED = 12345               # rows kept when the outputs exceed the budget: the same rows in every run of the same arguments


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float32 if a.dtype == np.float16 else np.float64)


def dump_outputs(directory, arrays, rank=0, world=1):
    """arrays: {name: tensor or array}, the batched ones with the rows as their first axis.  Writes DIR/<name>.npy in float32 or float64
    (the array's own precision where it is one of the two); with world > 1 ranks each writes <name>_rank<r>.npy within its share of the budget.
    If the arrays together exceed it, every batched array keeps the same fixed, seeded, sorted sample of rows.  Returns what was written."""
    suffix, budget = ("", DUMP_BUDGET_BYTES) if world == 1 else ("_rank%d" % rank, DUMP_BUDGET_BYTES // world)
    host = {k: _host(v) for k, v in arrays.items()}
    rows = max((a.shape[0] for a in host.values() if a.ndim >= 1), default=0)
    total = sum(a.nbytes for a in host.values())
    kept = None
    if total > budget and rows > 0:
        per_row = sum(a.nbytes // a.shape[0] for a in host.values() if a.ndim >= 1 and a.shape[0] == rows)
        fixed = total - per_row * rows
        n = max(1, min(rows, (budget - fixed) // max(1, per_row)))
        kept = np.sort(np.random.default_rng(SAMPLE_SEED).choice(rows, size=n, replace=False))
        host = {k: (a[kept] if a.ndim >= 1 and a.shape[0] == rows else a) for k, a in host.items()}
    os.makedirs(directory, exist_ok=True)
    files = []
    for k, a in host.items():
        path = os.path.join(directory, "%s%s.npy" % (k, suffix))
        np.save(path, a)
        files.append(os.path.basename(path))
    return {"dir": directory, "files": files, "rows": int(rows), "rows_written": int(rows if kept is None else len(kept)),
            "row_sample_seed": None if kept is None else SAMPLE_SEED}
