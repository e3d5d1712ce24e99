"""decode_batch(token_frames=True) against the plain call on the bench workload (4096 x T=1000 x V=1024, beam 100, 4-gram + the
bench's hot words, device logits). Per leg: ms per step and the library's split of the call (prune kernels, beam stage, whole
native call). For the token leg one more call runs with CTCDEC_HOST_TIMING=1, whose line splits the host part of the native
call into the copy of the chains back from the device and the C pass over them (replay: texts + token arrays); what is left of
the step outside the native call is Python (texts as str objects, the token arrays copied into numpy).
  python tools/token_frames_bench.py [--steps 10] [--warmup 2] [--batch 4096] [--out profiles/token_frames_bench.txt]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload's assets and batch, unchanged)


def _host_line(fn):
    """fn() with the library's stderr (CTCDEC_HOST_TIMING) captured -> its timing line"""
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
    lines = [ln for ln in text.splitlines() if "copy back" in ln]
    return lines[-1] if lines else text.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_frames_bench.txt"))
    args = ap.parse_args()
    import torch

    from pyctcdecode_amd import build_ctcdecoder

    cache = os.path.join(ROOT, "bench_cache") if os.access(ROOT, os.W_OK) else "/tmp/ctc_bench"
    lm, labels, hot = bench.build_assets(cache, 20000, 60000)
    xs = bench.make_batch(lm, labels, 0, args.batch, bench.T, 6.0, 16)
    dev = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    dec = build_ctcdecoder(labels, lm.path)
    kw = dict(beam_width=bench.BEAM, hotwords=hot)
    legs = {"plain": {}, "token_frames": {"token_frames": True}}
    res, outs = {}, {}
    for name, extra in legs.items():
        for _ in range(args.warmup):
            dec.decode_batch(None, dev, **kw, **extra)
        torch.cuda.synchronize()
        lib_ms = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            outs[name] = dec.decode_batch(None, dev, **kw, **extra)
            lib_ms.append(dec.last_timing_ms)
        dt = (time.perf_counter() - t0) / args.steps * 1000.0
        lib = np.mean(np.asarray(lib_ms), axis=0)
        res[name] = {"ms_per_step": round(dt, 3), "prune_ms": round(float(lib[0]), 3), "beam_ms": round(float(lib[1]), 3),
                     "native_call_ms": round(float(lib[2]), 3), "python_ms": round(dt - float(lib[2]), 3)}
        print(name, json.dumps(res[name]), flush=True)
    texts, tf = outs["token_frames"]
    host = _host_line(lambda: dec.decode_batch(None, dev, token_frames=True, **kw))
    m = re.search(r"copy back ([\d.]+) ms \((\d+) tokens\), replay ([\d.]+) ms", host)
    lines = [
        "decode_batch(token_frames=True) against the plain call: %d x T=%d x V=%d, beam %d, 4-gram + %d hot words, device "
        "float32 logits; %d steps after %d warm-up steps (tools/token_frames_bench.py)" % (
            args.batch, bench.T, bench.V, bench.BEAM, len(hot), args.steps, args.warmup),
        "",
        "%-14s %12s %10s %10s %15s %10s" % ("leg", "ms/step", "prune", "beam", "native call", "python"),
    ]
    for name in legs:
        r = res[name]
        lines.append("%-14s %12.3f %10.3f %10.3f %15.3f %10.3f" % (name, r["ms_per_step"], r["prune_ms"], r["beam_ms"],
                                                                  r["native_call_ms"], r["python_ms"]))
    ratio = res["token_frames"]["ms_per_step"] / res["plain"]["ms_per_step"]
    lines += [
        "",
        "ratio token_frames / plain: %.3f (target <= 1.3: %s)" % (ratio, "met" if ratio <= 1.3 else "NOT met"),
        "texts equal the plain call's: %s" % (texts == outs["plain"]),
        "tokens: %d (%.1f per utterance)" % (len(tf.label), len(tf.label) / max(1, len(tf))),
        "host split of one token_frames call (CTCDEC_HOST_TIMING): %s" % host,
    ]
    if m:
        lines.append("  chain copy %.3f ms for %s emission nodes (%.1f MB), C pass (replay: texts + tokens) %.3f ms" % (
            float(m.group(1)), m.group(2), int(m.group(2)) * 16 / 1e6, float(m.group(3))))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
