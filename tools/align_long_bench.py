"""Times forced alignment of long transcripts (align_long_batch: row_lse + ctc_viterbi_long, csrc/ctc_align_hip.hip) between HIP
events on the decode stream (last_align_long_timing_ms), medians of 3 steps after one warm-up:
  short     what score columns in device memory cost: align_long (one segment) next to align on the same batch, alternating --
            align_bench's shape (1000 frames x 1024 labels float32, targets of 408 labels) at 64 and 4096 utterances, and 256
            utterances of 2047 labels x 2100 frames
  segments  what checkpointing costs: 20000 frames x 32 labels, 5000 target labels, whose whole table is 50 MB -- one segment
            next to the balanced K
  hour      the case the call exists for: one utterance of 180000 frames x 32 labels float32 and 40000 target labels, which
            align refuses
Random logits and random targets: no kernel's time depends on the values. Every leg is a process of its own under `timeout`,
started by this one, which never opens the device; the first leg that fails ends the run.
  python tools/align_long_bench.py [--out profiles/align_long_bench.txt] [--steps 3] [--legs short64,short4096,short2047,segments,hour]"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEG_SECONDS = {"short64": 240, "short4096": 600, "short2047": 300, "segments": 240, "hour": 600}
DISTINCT = 256


def med(v):
    return float(np.median(v[1:]))  # (the first step is the warm-up)


def labels_of(V):
    return ["", " "] + [chr(0x4E00 + i) for i in range(V - 2)]  # the blank, the space and V - 2 distinct characters


def batch(n, T, V, L, seed):
    """n utterances of T x V float32 random logits on the device (min(n, 256) distinct ones repeated) and as many targets of L labels"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    d = min(n, DISTINCT)
    base = torch.randn((d, T, V), generator=g, device="cuda", dtype=torch.float32) * 3.0
    dev = base.repeat(n // d, 1, 1) if n > d else base
    rng = np.random.default_rng(seed)
    targets = []
    for _ in range(d):
        targets.append(rng.integers(1, V, size=L).tolist())  # (adjacent equal labels are rare enough for every shape here)
    return dev, targets * (n // d)


def alternate(dec, dev, targets, steps, long_kwargs):
    """align_batch and align_long_batch(**kw) for every kw, alternating: -> ([align kernel ms], {name: ([kernel ms], [native ms], plan)})"""
    vit, out = [], {name: ([], [], None) for name in long_kwargs}
    for _ in range(steps + 1):
        if vit is not None:
            try:
                dec.align_batch(dev, tokens=targets)
                vit.append(dec.last_align_timing_ms[2])
            except ValueError:
                vit = None  # (above align's limits)
        for name, kw in long_kwargs.items():
            dec.align_long_batch(dev, tokens=targets, **kw)
            ms = dec.last_align_long_timing_ms
            out[name][0].append(ms[2]), out[name][1].append(ms[3])
            out[name] = (out[name][0], out[name][1], dec.last_align_long_plan[0])
    return vit, out


def leg_short(n, T, V, L, steps):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(labels_of(V))
    dev, targets = batch(n, T, V, L, 1)
    vit, out = alternate(dec, dev, targets, steps, {"whole": {}})
    kern, native, plan = out["whole"]
    return ["%d utterances of %d frames x %d labels float32, targets of %d labels (plan %s, %d launch(es)):" % (n, T, V, L, plan, dec.last_align_long_launches),
            "  ctc_viterbi       %10.3f ms  (align_batch, columns in LDS)" % med(vit),
            "  ctc_viterbi_long  %10.3f ms  (align_long_batch, columns in device memory; native call %.3f ms)" % (med(kern), med(native)),
            "  ctc_viterbi_long / ctc_viterbi: %.2f" % (med(kern) / med(vit))]


def leg_segments(steps):
    from pyctcdecode_amd import build_ctcdecoder

    T, V, L = 20000, 32, 5000
    K = min(T, math.isqrt(32 * T - 1) + 1)  # ceil(sqrt(32 T))
    dec = build_ctcdecoder(labels_of(V))
    dev, targets = batch(1, T, V, L, 2)
    _vit, out = alternate(dec, dev, targets, steps, {"whole": {}, "cut": {"_segment_frames": K}})
    (k1, n1, p1), (k2, n2, p2) = out["whole"], out["cut"]
    b1, b2 = dec._align_long_plan(T, L, 1 << 30, 0)[2], dec._align_long_plan(T, L, 1 << 30, K)[2]
    return ["one utterance of %d frames x %d labels float32, %d target labels:" % (T, V, L),
            "  one segment  plan %-12s %11d bytes  ctc_viterbi_long %10.3f ms  native call %10.3f ms" % (p1, b1, med(k1), med(n1)),
            "  balanced K   plan %-12s %11d bytes  ctc_viterbi_long %10.3f ms  native call %10.3f ms" % (p2, b2, med(k2), med(n2)),
            "  balanced K / one segment: %.2f  (the second pass repeats every frame's work; the back-trace runs once in both)" % (med(k2) / med(k1))]


def leg_hour(steps):
    from pyctcdecode_amd import build_ctcdecoder

    T, V, L = 180000, 32, 40000
    dec = build_ctcdecoder(labels_of(V))
    dev, targets = batch(1, T, V, L, 3)
    try:
        dec.align_batch(dev, tokens=targets)
        refusal = "align_batch accepted it"
    except ValueError as e:
        refusal = "align_batch: ValueError: %s" % e
    wall, kern, native, lse = [], [], [], []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        a = dec.align_long_batch(dev, tokens=targets)[0]
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = dec.last_align_long_timing_ms
        lse.append(ms[1]), kern.append(ms[2]), native.append(ms[3])
    K, n = dec.last_align_long_plan[0]
    nbytes = dec._align_long_plan(T, L, 1 << 30, 0)[2]
    whole = dec._align_long_plan(T, L, 1 << 62, 0)[2]
    assert len(a.path) == T and len(a.token_frames) == sum(1 for c in targets[0] if c != 1) and n > 1  # (label 1, the space, is no token)
    return ["one utterance of %d frames x %d labels float32 (%.1f MB of logits), %d target labels:" % (T, V, T * V * 4 / 1e6, L),
            "  %s" % refusal,
            "  plan: %d segments of %d frames, %d bytes (%.1f MB; one segment would take %.2f GB)" % (n, K, nbytes, nbytes / 1e6, whole / 1e9),
            "  row_lse           %10.3f ms" % med(lse),
            "  ctc_viterbi_long  %10.3f ms  (two passes over the frames and the back-trace: %.3f ms per pass, %.2f us per frame and pass)"
            % (med(kern), med(kern) / 2, med(kern) * 1e3 / (2 * T)),
            "  native call       %10.3f ms   align_long_batch %10.3f ms" % (med(native), med(wall))]


def run_leg(leg, steps):
    if leg == "short64":
        return leg_short(64, 1000, 1024, 408, steps)
    if leg == "short4096":
        return leg_short(4096, 1000, 1024, 408, steps)
    if leg == "short2047":
        return leg_short(256, 2100, 1024, 2047, steps)
    if leg == "segments":
        return leg_segments(steps)
    if leg == "hour":
        return leg_hour(steps)
    raise SystemExit("unknown leg %r" % leg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_long_bench.txt"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--legs", default="short64,short4096,short2047,segments,hour")
    ap.add_argument("--leg", default=None, help="(a child of this tool) run one leg in this process and print its lines")
    args = ap.parse_args()
    if args.leg:
        print("\n".join(run_leg(args.leg, args.steps)))
        return
    lines = ["forced alignment of long transcripts, kernels between HIP events; %d steps after one warm-up, medians; each leg a process of its own" % args.steps]
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
