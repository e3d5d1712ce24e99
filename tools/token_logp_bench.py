"""decode_batch(confidence="mean") against the plain and the token_frames=True call on the bench workload (4096 x T=1000 x
V=1024, beam 100, 4-gram + the bench's hot words, device float32 logits). Per leg: median, smallest and largest ms per step and
the library's split of the call. For the confidence leg one more call runs with CTCDEC_HOST_TIMING=1, whose line gives the
token_logp kernel's time from HIP events, the pack + upload of the tokens and the download of the values.

The comparison against the parent commit needs the parent built in a tree of its own and run in the same GPU visit, one
process per tree (one library per process):
  python tools/token_logp_bench.py --root <parent tree> --json parent.json      # plain and token_frames legs only
  python tools/token_logp_bench.py --parent parent.json [--out profiles/token_logp_bench.txt]
  [--steps 10] [--warmup 3] [--batch 4096]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_lines(fn):
    """fn() with the library's stderr (CTCDEC_HOST_TIMING) captured -> its timing lines"""
    os.environ["CTCDEC_HOST_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["CTCDEC_HOST_TIMING"]
        f.seek(0)
        text = f.read().decode("utf-8", "replace")
    return [ln for ln in text.splitlines() if ln.startswith("[ctcdec host]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--root", default=ROOT, help="the tree whose pyctcdecode_amd is measured (default: this one)")
    ap.add_argument("--json", default=None, help="write the legs' figures here (what --parent reads)")
    ap.add_argument("--parent", default=None, help="the --json file of the parent commit's run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_logp_bench.txt"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import inspect

    import torch

    import bench  # (the workload's assets and batch, unchanged)
    from pyctcdecode_amd import build_ctcdecoder

    assert os.path.dirname(os.path.abspath(bench.__file__)) == root, bench.__file__
    cache = os.path.join(ROOT, "bench_cache") if os.access(ROOT, os.W_OK) else "/tmp/ctc_bench"
    lm, labels, hot = bench.build_assets(cache, 20000, 60000)
    xs = bench.make_batch(lm, labels, 0, args.batch, bench.T, 6.0, 16)
    dev = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    dec = build_ctcdecoder(labels, lm.path)
    kw = dict(beam_width=bench.BEAM, hotwords=hot)
    legs = {"plain": {}, "token_frames": {"token_frames": True}}
    has_conf = "confidence" in inspect.signature(dec.decode_batch).parameters
    if has_conf:
        legs["confidence"] = {"confidence": "mean"}
    res, outs = {}, {}
    for name, extra in legs.items():
        for _ in range(args.warmup):
            dec.decode_batch(None, dev, **kw, **extra)
        torch.cuda.synchronize()
        step_ms, lib_ms = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            outs[name] = dec.decode_batch(None, dev, **kw, **extra)
            step_ms.append((time.perf_counter() - t0) * 1000.0)
            lib_ms.append(dec.last_timing_ms)
        lib = np.median(np.asarray(lib_ms), axis=0)
        res[name] = {"median_ms": round(float(np.median(step_ms)), 3), "min_ms": round(min(step_ms), 3),
                     "max_ms": round(max(step_ms), 3), "prune_ms": round(float(lib[0]), 3), "beam_ms": round(float(lib[1]), 3),
                     "native_call_ms": round(float(lib[2]), 3)}
        print(name, json.dumps(res[name]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"root": root, "steps": args.steps, "warmup": args.warmup, "batch": args.batch, "legs": res}, f, indent=1)
    if not has_conf:
        return
    texts, tf = outs["confidence"]
    host = _host_lines(lambda: dec.decode_batch(None, dev, confidence="mean", **kw))
    head = ("decode_batch(confidence=\"mean\") against the plain and the token_frames=True call: %d x T=%d x V=%d, beam %d, 4-gram + "
            "%d hot words, device float32 logits; %d timed steps after %d warm-up steps, ms per step as median (min .. max) "
            "(tools/token_logp_bench.py)" % (args.batch, bench.T, bench.V, bench.BEAM, len(hot), args.steps, args.warmup))
    fmt = "%-22s %10s %22s %10s %10s %14s"
    lines = [head, "", fmt % ("leg", "median", "(min .. max)", "prune", "beam", "native call")]

    def row(label, r):
        return fmt % (label, "%.3f" % r["median_ms"], "(%.3f .. %.3f)" % (r["min_ms"], r["max_ms"]), "%.3f" % r["prune_ms"],
                      "%.3f" % r["beam_ms"], "%.3f" % r["native_call_ms"])

    parent = None
    if args.parent:
        with open(args.parent) as f:
            parent = json.load(f)
        for name in ("plain", "token_frames"):
            lines.append(row("parent " + name, parent["legs"][name]))
    for name in legs:
        lines.append(row(name, res[name]))
    lines.append("")
    if parent:
        lines.append("against the parent commit, built and run in the same GPU visit (%d steps after %d warm-up steps):" % (
            parent["steps"], parent["warmup"]))
        for name in ("plain", "token_frames"):
            ratio = res[name]["median_ms"] / parent["legs"][name]["median_ms"]
            lines.append("  (a) %-12s this tree / parent: %.4f (within 3 %%: %s)" % (name, ratio, "yes" if abs(ratio - 1) <= 0.03 else "NO"))
        ratio = res["confidence"]["median_ms"] / parent["legs"]["token_frames"]["median_ms"]
        lines.append("  (b) confidence / parent token_frames: %.4f%s" % (ratio, "" if ratio <= 1.15 else " (above 1.15: see the split below)"))
    lines += [
        "confidence / token_frames of this tree: %.4f" % (res["confidence"]["median_ms"] / res["token_frames"]["median_ms"]),
        "texts equal the plain call's: %s" % (texts == outs["plain"]),
        "tokens: %d (%.1f per utterance); up %.1f MB (12 B per token), down %.1f MB (8 B per token)" % (
            len(tf.label), len(tf.label) / max(1, len(tf)), len(tf.label) * 12 / 1e6, len(tf.label) * 8 / 1e6),
        "host split of one confidence call (CTCDEC_HOST_TIMING; the kernel's time is from HIP events):",
    ] + ["  " + ln for ln in host]
    m = re.search(r"kernel ([\d.]+) ms", " ".join(ln for ln in host if "token confidences" in ln))
    if m:
        lines.append("token_logp kernel: %.3f ms" % float(m.group(1)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
