"""Writes tests/golden/ref_tracking.npz: reference-tracking instances (tests/refs_cases.py, kinds a-f) solved by the REFERENCE's own
`solve_mpc` with its two generators (REF:61-70, REF:72-109) replaced by functions that return the supplied arrays -- what a user
of the reference who edits `x_ref` / `foot_ref` runs.  The QP it hands to cvxopt (REF:297) is captured and solved by the oracle
(oracle/gen_golden.py `_Capture`).  Run on a machine that has the reference:

    python -m tests.gen_ref_tracking

Per horizon h (keys prefixed "h<h>_"): the inputs (fp32-representable), x_ref (n,13,h), foot_ref (n,6,h), kind, the captured
q, hvec (the inequality right-hand side `h` of REF:297), b, the certified optimum (controls, states) and, for the first two
instances, P / G / A as triplets (<name><i>_rc: rows and columns, <name><i>_v: values)."""
import contextlib
import io
import os

import numpy as np

from tests import refs_cases as rc

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tracking.npz")
PLAN = [(10, 18, 101), (16, 6, 116), (20, 6, 120)]          # (h, instances: kinds a-f in turn, seed)


def main():
    from oracle import gen_golden as gg
    ref, cap = gg.load_reference()
    out = {}
    for h, n, seed in PLAN:
        s = rc.make_batch(n, h, seed, kinds=rc.KINDS)
        cols = {k: [] for k in ("q", "hvec", "b", "controls", "states", "certified")}
        for i in range(n):
            mpc, biped = ref.MPC(), ref.Biped()
            mpc.h, mpc.x_cmd = h, np.array(s["x_cmd"][i], float)
            with rc.supplied(ref, s["x_ref"][i], s["foot_ref"][i]), contextlib.redirect_stdout(io.StringIO()):   # (REF:190-192 print)
                ref.solve_mpc(np.array(s["x_fb"][i], float), float(s["t"][i]), np.array(s["foot"][i], float), mpc, biped,
                              np.array(s["contact"][i], int))
            qp = cap.last
            k = qp["info"]["kkt"]
            cols["q"].append(qp["q"]); cols["hvec"].append(qp["h"]); cols["b"].append(qp["b"])
            cols["controls"].append(qp["z"][13 * h:].reshape(h, 12)); cols["states"].append(qp["z"][:13 * h].reshape(h, 13))
            cols["certified"].append(bool(qp["info"]["polished"]) and max(k["stationarity"], k["primal_ineq"], k["complementarity"]) <= 1e-7)
            if i < 2:
                for name in ("P", "G", "A"):
                    out[f"h{h}_{name}{i}_rc"], out[f"h{h}_{name}{i}_v"] = gg.sparse_triplets(qp[name])
        for key in ("x_fb", "foot", "contact", "phase", "t", "x_cmd", "x_ref", "foot_ref", "kind"):
            out[f"h{h}_{key}"] = s[key]
        out[f"h{h}_half"] = np.array(s["half"])
        for key, v in cols.items():
            out[f"h{h}_{key}"] = np.stack(v)
        print(f"h = {h}: {n} instances, certified {int(np.sum(cols['certified']))}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
