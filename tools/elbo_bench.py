"""Cost of the variational lower bound (vlgp_elbo) beside the E-step it follows, on a bench.py workload.

One process, one box.  Prints one JSON line:
- sweep_ms: one E-step sweep of this run, median(e_elapsed) / Eniter over --steps EM iterations after --warmup;
- elbo_segments_ms / elbo_trials_ms: device-synchronised wall time of Engine.elbo (launches, the copy of the terms to
  the host and the wait for it) on the segment set at its steady-state ranks and on the full-length trials with their
  own prior factors, median of --reps after one warm-up call;
- em_ms_track_off / em_ms_track_on: median EM iteration time of fresh sessions run alternately without and with
  track_elbo, --ab-iters iterations each from cold (the protocol of tools/ab_old_new.sh), --ab-rounds rounds.
    python tools/elbo_bench.py [--workload C3 --warmup 5 --steps 20 --reps 20 --ab-iters 30 --ab-rounds 2]
(--only-elbo: the warm-up and the elbo calls alone, for a kernel trace under rocprofv3.)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ab-iters", type=int, default=30)
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--only-elbo", action="store_true")
    args = ap.parse_args()
    import bench
    from vlgp_amd import engine as E
    from vlgp_amd.api import SET_SEGMENTS, SET_TRIALS, FitSession

    trials, a0, b0, (n_trials, n_bins, N, L) = bench.build_inputs(args.workload)
    _, lik = bench.workload_extras(args.workload, n_trials)
    extra = {"lik": lik} if lik else {}

    def session(track, iters):
        mine = [dict(t) for t in trials]
        return FitSession(mine, L, verbose=False, a=a0.copy(), b=b0.copy(), max_iter=iters, min_iter=iters,
                          track_elbo=track, **extra)

    def timed_elbo(eng, sid):
        eng.elbo(sid)  # warm-up: code object, buffer
        out = []
        for _ in range(args.reps):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.elbo(sid)
            out.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(out), out

    total = args.warmup + (0 if args.only_elbo else args.steps)
    sess = session(False, total)
    out = {"workload": args.workload, "units": len(sess.segs), "window": sess.config["window"], "N": N, "L": L}
    try:
        eng = sess.eng
        for _ in range(total):
            sess.em_iteration()
        if not args.only_elbo:
            e = sess.runtime["e_elapsed"][args.warmup:]
            out["e_step_ms"] = 1e3 * statistics.median(e)
            out["sweep_ms"] = out["e_step_ms"] / sess.config["Eniter"]
        out["ranks_segments"] = [int(r) for r in eng.prior_ranks(sess.config["window"])]
        out["elbo_segments_ms"], runs = timed_elbo(eng, SET_SEGMENTS)
        out["elbo_segments_runs_ms"] = [round(r, 4) for r in runs]
        # the full-length trials under their own factors, as FitSession.finish sets them up
        if sess.segs is not sess.dev_trials:
            eng.merge(SET_SEGMENTS)
        E.make_cholesky(sess.dev_trials, sess.params, sess.config)
        E.update_w(sess.dev_trials, sess.params, sess.config)
        E.update_v(sess.dev_trials, sess.params, sess.config)
        out["ranks_trials"] = eng.unit_ranks(SET_TRIALS).max(axis=0).tolist()
        out["elbo_trials_ms"], runs = timed_elbo(eng, SET_TRIALS)
        out["elbo_trials_runs_ms"] = [round(r, 4) for r in runs]
        if "sweep_ms" in out:
            out["elbo_segments_in_sweeps"] = out["elbo_segments_ms"] / out["sweep_ms"]
    finally:
        sess.close()
    if not args.only_elbo:
        ab = {False: [], True: []}
        for _ in range(args.ab_rounds):
            for track in (False, True):
                s = session(track, args.ab_iters)
                try:
                    for _ in range(args.ab_iters):
                        s.em_iteration()
                    ab[track].append(1e3 * statistics.median(s.runtime["em_elapsed"]))
                finally:
                    s.close()
        out["em_ms_track_off"] = statistics.median(ab[False])
        out["em_ms_track_on"] = statistics.median(ab[True])
        out["em_ms_track_off_runs"], out["em_ms_track_on_runs"] = ab[False], ab[True]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
