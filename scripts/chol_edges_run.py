"""GPU box: every case of tests/chol_reference.py::cases() through the four forms of dense_chol.hip (dense solve, planned dense solve, tile-sparse solve,
inverse), with whatever CCM_CHOL_* switches the environment carries (they are read once per process, hence a process per variant); every result goes into
ONE .npz.  tests/test_chol_edges_gpu.py runs the same list in its own process and in children with CCM_CHOL_DIAG=columns and CCM_CHOL_CHAIN=split.
Keys: <form>__<case>__x / __info (tile: also __levels, __tiles); after a case that must fail, the small SPD system of chol_reference.recheck_case() is solved
by the same form on the same context: __re_x, __re_info.
usage: chol_edges_run.py <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from tests import chol_reference as ref

FORMS = ("dense", "planned", "tile", "inverse")
SOLVES = ("dense", "planned", "tile")


def call(ctx, form, A, b):
    """one hook call -> dict(x, info[, levels, tiles]); x is the inverse for form "inverse".  The wrappers raise unless the call returned CCM_OK."""
    from ccm_slam_amd import optimizer
    if form == "dense":
        x, info = optimizer.debug_dense_solve(ctx, A, b)
    elif form == "planned":
        x, info = optimizer.debug_planned_solve(ctx, A, b)
    elif form == "tile":
        x, info, levels, tiles = optimizer.debug_tile_solve(ctx, A, b)
        return dict(x=x, info=info, levels=levels, tiles=tiles)
    else:
        x, info = optimizer.debug_dense_inverse(ctx, A)
    return dict(x=x, info=info)


def run_cases(ctx):
    out = {}
    Ar, br = ref.recheck_case()
    for c in ref.cases():
        for form in FORMS:
            for k, v in call(ctx, form, c["A"], c["b"]).items():
                out[f"{form}__{c['name']}__{k}"] = v
            if c["kind"] != "ok":
                r = call(ctx, form, Ar, br)
                out[f"{form}__{c['name']}__re_x"], out[f"{form}__{c['name']}__re_info"] = r["x"], r["info"]
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == "__main__":
    from ccm_slam_amd._lib import Context
    ctx = Context(0)
    np.savez(sys.argv[1], **run_cases(ctx))
    ctx.close()
