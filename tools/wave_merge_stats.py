"""How often do the candidates of a wave-kernel frame merge, and what does finding that out cost? (CPU, exact counts)
Decodes bench utterances through the statistics build of the simulator (tests/sim, -DCTC_STATS) and reads its per-frame `ST` lines:
live beams N, survivors ns, pool entries, kept beams, match-table rounds, candidates that joined another candidate's group,
pass1 calls, loser-loop steps (beam_wave.h: wave_match).
  python tools/wave_merge_stats.py [n_utts=6] [first=0]      (about a minute per 8 utterances and core)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.weigh_predictors import build_stats_lib, sim_stats  # noqa: E402


def collect(first, n):
    """{utterance: [ST tuple per full frame]}"""
    procs = [sim_stats(first + k, min(8, n - k)) for k in range(0, n, 8)]
    utts, cur = {}, None
    for p in procs:
        for line in p.stderr:
            if line.startswith("UTT"):
                cur = int(line.split()[1])
                utts[cur] = []
            elif line.startswith("ST") and cur is not None:
                utts[cur].append(tuple(map(int, line.split()[1:])))
        if p.wait() != 0:
            raise RuntimeError("the simulator run of utterances %d.. failed" % first)
    return utts


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    from tests.sim import build_sim

    os.makedirs(build_sim.OUT_DIR, exist_ok=True)
    build_stats_lib()
    utts = collect(first, n)
    r = np.array([t for u in sorted(utts) for t in utts[u]], dtype=np.int64)
    if r.shape[1] < 8:
        raise SystemExit("the ST lines carry no merge counters: the statistics library is stale")
    N, ns, rounds, members, pass1, loop = r[:, 0], r[:, 1], r[:, 4], r[:, 5], r[:, 6], r[:, 7]
    big = np.where(N > 64, ns, 0)  # (more than 64 live beams: one pass_big per label, no pass1)
    passes = pass1 + big
    cand = N * ns
    f = float(len(r))
    print("%d utterances (%d..%d), %d full frames" % (len(utts), first, first + n - 1, len(r)))
    print("| per full frame (mean) | value |")
    print("|---|---|")
    print("| candidates (N x ns) | %.1f |" % (cand.sum() / f))
    print("| candidates that are their own representative | %.1f |" % ((cand - members).sum() / f))
    print("| frames with any merge at all | %.1f %% |" % (100.0 * (members > 0).sum() / f))
    print("| `pass1` calls | %.2f |" % (pass1.sum() / f))
    print("| `pass_big` calls | %.3f |" % (big.sum() / f))
    print("| match-table rounds per pass | %.2f |" % (rounds.sum() / max(1.0, float(passes.sum()))))
    print("| loser-loop steps per pass | %.2f |" % (loop.sum() / max(1.0, float(passes.sum()))))
    print("| merged candidates, all frames | %d |" % members.sum())


if __name__ == "__main__":
    main()
