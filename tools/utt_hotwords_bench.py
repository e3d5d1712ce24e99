"""Per-utterance hot words on the bench workload (4096 x T=1000 x V=1024, beam 100, 4-gram): three legs in one process --
  shared    the bench's 25-word list, shared by the batch (the headline call)
  per_utt   the same list given once per utterance (deduplicated to one set: the call-wide path)
  distinct  4096 distinct lists of 10-25 words (4096 sets: ctcdec_set_hotword_sets, hot_tok_build)
For each: ms per decode_batch step (device logits), the Python side of the hot words (normalising, deduplicating, packing) and
the library's own split of the call (prune kernels, beam stage, whole native call). The hot_tok_build kernel's time comes from
a separate kernel trace:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/utt_hotwords_bench.py --legs distinct
  python tools/utt_hotwords_bench.py [--steps 10] [--warmup 2] [--batch 4096] [--legs shared,per_utt,distinct]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload's assets and batch, unchanged)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--legs", default="shared,per_utt,distinct")
    args = ap.parse_args()
    import torch

    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.decoder import BeamSearchDecoderCTC

    cache = os.path.join(ROOT, "bench_cache") if os.access(ROOT, os.W_OK) else "/tmp/ctc_bench"
    lm, labels, hot = bench.build_assets(cache, 20000, 60000)
    xs = bench.make_batch(lm, labels, 0, args.batch, bench.T, 6.0, 16)
    dev = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    dec = build_ctcdecoder(labels, lm.path)
    rng = np.random.default_rng(11)
    words = list(lm.words)
    distinct = [[words[int(i)] for i in rng.choice(len(words), size=int(rng.integers(10, 26)), replace=False)]
                for _ in range(args.batch)]
    legs = {"shared": (hot, 10.0), "per_utt": ([list(hot) for _ in range(args.batch)], 10.0), "distinct": (distinct, 10.0)}
    out = {"workload": "%d x T=%d x V=%d, beam %d" % (args.batch, bench.T, bench.V, bench.BEAM), "legs": {}}
    ref_texts = None
    for name in args.legs.split(","):
        hw, w = legs[name]
        t0 = time.perf_counter()
        for _ in range(5):
            BeamSearchDecoderCTC._resolve_hot(dec, hw, w, args.batch)
        py_ms = (time.perf_counter() - t0) / 5 * 1000.0
        for _ in range(args.warmup):
            texts = dec.decode_batch(None, dev, beam_width=bench.BEAM, hotwords=hw, hotword_weight=w)
        torch.cuda.synchronize()
        lib_ms = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            texts = dec.decode_batch(None, dev, beam_width=bench.BEAM, hotwords=hw, hotword_weight=w)
            lib_ms.append(dec.last_timing_ms)
        dt = (time.perf_counter() - t0) / args.steps
        lib = np.mean(np.asarray(lib_ms), axis=0)
        if name == "shared":
            ref_texts = texts
        out["legs"][name] = {"ms_per_step": round(dt * 1000.0, 3), "python_hot_ms": round(py_ms, 3),
                             "prune_ms": round(float(lib[0]), 3), "beam_ms": round(float(lib[1]), 3),
                             "native_call_ms": round(float(lib[2]), 3),
                             "same_texts_as_shared": (texts == ref_texts) if ref_texts is not None else None}
        print(name, json.dumps(out["legs"][name]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
