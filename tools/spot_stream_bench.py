"""Kernel time of one SpotStreams.feed on cuda:0: ctc_spot_chunk packed, the same with CTCDEC_SPOT_STREAM_WIDTH=64 (a wavefront
per phrase), and spot_batch on the same chunks taken as separate utterances (ctc_spot_wave: what the library could do with
these frames and phrases without sessions). The three alternate in one process; medians of the kernels' HIP-event times after
a warm-up. Shapes: streams x keywords of 8 labels x chunks of 32 frames x 1024 labels, float32 device tensors.

    python tools/spot_stream_bench.py [--reps 15] [--warmup 3] > profiles/spot_stream_bench.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyctcdecode_amd import build_ctcdecoder  # noqa: E402

V, FRAMES, LABELS = 1024, 32, 8
SHAPES = ((256, 8), (1024, 48))  # (streams, keywords each)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spot_stream_bench.py measures on cuda:0"
    dec = build_ctcdecoder(["", " "] + [chr(0x4E00 + k) for k in range(V - 2)])  # (the blank, the space, V - 2 characters)
    print("ctc_spot_chunk against ctc_spot_wave: kernel ms of one feed (HIP events), medians of %d after %d warm-up feeds; %d labels, "
          "chunks of %d frames, keywords of %d labels, float32 device tensors" % (args.reps, args.warmup, V, FRAMES, LABELS))
    for n_streams, n_keys in SHAPES:
        rng = np.random.default_rng(n_streams)
        keys = [[int(c) for c in rng.integers(2, V, LABELS)] for _ in range(n_keys)]
        chunks = [torch.from_numpy(rng.standard_normal(((args.reps + args.warmup) * FRAMES, V)).astype(np.float32)).cuda()
                  for _ in range(min(n_streams, 16))]
        times = {"packed": [], "width64": [], "spot_batch": []}
        waves = {}
        sessions = {"packed": dec.spot_streams(tokens=keys, n_streams=n_streams), "width64": dec.spot_streams(tokens=keys, n_streams=n_streams)}
        for k in range(args.reps + args.warmup):
            feed = [chunks[u % len(chunks)][k * FRAMES:(k + 1) * FRAMES] for u in range(n_streams)]
            for name in ("packed", "width64", "spot_batch"):
                if name == "spot_batch":
                    dec.spot_batch(feed, tokens=[keys] * n_streams)
                    ms = dec.last_spot_timing_ms[2]
                else:
                    if name == "width64":
                        os.environ["CTCDEC_SPOT_STREAM_WIDTH"] = "64"
                    sessions[name].feed(feed)
                    os.environ.pop("CTCDEC_SPOT_STREAM_WIDTH", None)
                    ms, waves[name] = dec.last_spot_stream_timing_ms[2], sum(dec.last_spot_stream_launched)
                if k >= args.warmup:
                    times[name].append(ms)
        for s in sessions.values():
            s.close()
        med = {name: statistics.median(v) for name, v in times.items()}
        print("%5d streams x %2d keywords = %6d items: packed %8.3f ms (%6d wavefronts, min %.3f max %.3f)  width 64 %8.3f ms (%6d wavefronts)  "
              "spot_batch %8.3f ms   packed / width 64 = %.2f   packed / spot_batch = %.2f"
              % (n_streams, n_keys, n_streams * n_keys, med["packed"], waves["packed"], min(times["packed"]), max(times["packed"]),
                 med["width64"], waves["width64"], med["spot_batch"], med["packed"] / med["width64"], med["packed"] / med["spot_batch"]))


if __name__ == "__main__":
    main()
