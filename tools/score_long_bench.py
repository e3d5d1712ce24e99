"""Times the likelihood of long transcripts (score_long_batch: row_lse + ctc_forward_tile, csrc/ctc_align_hip.hip) between HIP
events on the decode stream (last_score_long_timing_ms), medians of 3 steps after one warm-up, each next to its yardstick on
the same device tensors in the same process:
  hour       one utterance of 180000 frames x 32 labels float32 and 40000 labels: one pass of ctc_viterbi_long (half of
             align_long_batch's two), then score_long at tile_frames 64, 128, 256, 512, 1024 and at the library's plan
  short64,   align_bench's shape (1000 frames x 1024 labels float32, hypotheses of 408 labels, one tile each) at 64 and 4096
  short4096  utterances: score_batch next to score_long_batch, alternating
  short2047  256 utterances of 2100 frames x 1024 labels with 2047 labels, the largest shape both calls take: ctc_forward<1024>
             next to four state blocks
Random logits and random labels: no kernel's time depends on the values. Every leg is a process of its own under `timeout`,
started by this one, which never opens the device; the first leg that fails ends the run.
  python tools/score_long_bench.py [--out profiles/score_long_bench.txt] [--steps 3] [--legs hour,short64,short4096,short2047]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from align_long_bench import batch, labels_of, med  # noqa: E402

LEG_SECONDS = {"hour": 600, "short64": 240, "short4096": 600, "short2047": 300}
HOUR_TILE_FRAMES = (64, 128, 256, 512, 1024)


def leg_hour(steps):
    from pyctcdecode_amd import build_ctcdecoder

    T, V, L = 180000, 32, 40000
    dec = build_ctcdecoder(labels_of(V))
    dev, targets = batch(1, T, V, L, 3)
    hyps = [[t] for t in targets]
    try:
        dec.score_batch(dev, tokens=hyps)
        refusal = "score_batch accepted it"
    except ValueError as e:
        refusal = "score_batch: ValueError: %s" % e
    vit = []
    for _ in range(steps + 1):
        dec.align_long_batch(dev, tokens=targets)
        vit.append(dec.last_align_long_timing_ms[2] / 2)
    lines = ["one utterance of %d frames x %d labels float32 (%.1f MB of logits), one hypothesis of %d labels:" % (T, V, T * V * 4 / 1e6, L),
             "  %s" % refusal,
             "  ctc_viterbi_long, one pass  %10.3f ms  (half of align_long_batch's two: one workgroup)" % med(vit),
             "  tile_frames  state x time blocks  diagonals  tiles  widest  bytes     fill + ctc_forward_tile   / one pass  native call"]
    scores = set()
    for fb in HOUR_TILE_FRAMES + (0,):
        kern, native = [], []
        for _ in range(steps + 1):
            scores.add(dec.score_long_batch(dev, tokens=hyps, _tile_frames=fb)[0][0].logp)
            kern.append(dec.last_score_long_timing_ms[2]), native.append(dec.last_score_long_timing_ms[3])
        gb, f, ni, nj, nbytes = dec.last_score_long_plan[0]
        lines.append("  %-11s  %5d x %-5d  %17d  %5d  %6d  %8d  %14.3f ms  %14.3f  %10.3f ms"
                     % ("%d%s" % (f, "" if fb else " (plan)"), ni, nj, dec.last_score_long_launches, dec.last_score_long_tiles,
                        dec.last_score_long_widest, nbytes, med(kern), med(kern) / med(vit), med(native)))
    assert len(scores) == 1, scores  # (the same bits at every tile shape)
    lines.append("  logp %.6f at every tile shape" % scores.pop())
    return lines


def leg_short(n, T, V, L, steps):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(labels_of(V))
    dev, targets = batch(n, T, V, L, 1)
    hyps = [[t] for t in targets]
    fwd, tile, native = [], [], []
    for _ in range(steps + 1):
        a = dec.score_batch(dev, tokens=hyps)
        fwd.append(dec.last_score_timing_ms[2])
        b = dec.score_long_batch(dev, tokens=hyps)
        tile.append(dec.last_score_long_timing_ms[2]), native.append(dec.last_score_long_timing_ms[3])
    assert [h[0].logp for h in a] == [h[0].logp for h in b]
    gb, f, ni, nj, _bytes = dec.last_score_long_plan[0]
    return ["%d utterances of %d frames x %d labels float32, one hypothesis of %d labels each (%d x %d tiles of %d frames, %d diagonals):"
            % (n, T, V, L, ni, nj, f, dec.last_score_long_launches),
            "  ctc_forward       %10.3f ms  (score_batch, one workgroup per hypothesis)" % med(fwd),
            "  ctc_forward_tile  %10.3f ms  (score_long_batch, fill included; native call %.3f ms)" % (med(tile), med(native)),
            "  ctc_forward_tile / ctc_forward: %.2f" % (med(tile) / med(fwd))]


def run_leg(leg, steps):
    if leg == "hour":
        return leg_hour(steps)
    if leg in ("short64", "short4096"):
        return leg_short(int(leg[5:]), 1000, 1024, 408, steps)
    if leg == "short2047":
        return leg_short(256, 2100, 1024, 2047, steps)
    raise SystemExit("unknown leg %r" % leg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_long_bench.txt"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--legs", default="hour,short64,short4096,short2047")
    ap.add_argument("--leg", default=None, help="(a child of this tool) run one leg in this process and print its lines")
    args = ap.parse_args()
    if args.leg:
        print("\n".join(run_leg(args.leg, args.steps)))
        return
    lines = ["likelihood of long transcripts, kernels between HIP events; %d steps after one warm-up, medians; each leg a process of its own" % args.steps]
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(LEG_SECONDS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(args.steps)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            lines.append("%s: exit status %d; nothing more was started\n%s" % (leg, done.returncode, done.stderr[-2000:]))
            break
        lines += done.stdout.rstrip("\n").splitlines()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    sys.exit(0 if done.returncode == 0 else 1)


if __name__ == "__main__":
    main()
