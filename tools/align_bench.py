"""Times forced alignment (align_batch: row_lse + ctc_viterbi, csrc/ctc_align_hip.hip) at the bench shape -- 4096 utterances
of 1000 frames x 1024 labels, float32, each aligned to its own decoded tokens -- and at 64 utterances, with the plain
decode_batch step of the same process for scale. Kernel times are HIP events on the decode stream (ctcdec_alignment_timing).
  python tools/align_bench.py [--out profiles/align_bench.txt] [--steps 3]
The 4096 utterances are 256 distinct ones repeated: neither kernel's time depends on the rows being distinct."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

T, V, DISTINCT = 1000, 1024, 256
HBM_PEAK = 8.0e12  # bytes / s
_G = {}


def _gen(u):
    g = _G
    return synth.d_words(4, u, T, g["labels"], True, g["words"], g["sentences"], len(g["labels"]), boost=6.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    lm = synth.SynthLM(os.path.join(ROOT, "bench_cache"), 2000, 6000, order=3, seed=7, max_ngrams={2: 60_000, 3: 120_000})
    labels = synth.make_bpe_vocab(lm.words, size=V - 1)
    _G.update(labels=labels, words=lm.words, sentences=lm.sentences)
    import multiprocessing as mp

    with mp.get_context("fork").Pool(args.procs) as pool:  # (forked before the HIP runtime exists in this process)
        base = np.stack(pool.map(_gen, range(DISTINCT), chunksize=4))
        pool.close()
        pool.join()
    import torch

    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(labels, lm.path)
    base_dev = torch.from_numpy(base).cuda()
    lines = ["forced alignment, %d frames x %d labels float32 per utterance, targets = the utterance's own decoded tokens; "
             "%d steps after one warm-up, medians" % (T, V, args.steps)]
    for n in (4096, 64):
        dev = base_dev.repeat(n // DISTINCT, 1, 1) if n > DISTINCT else base_dev[:n].contiguous()
        torch.cuda.synchronize()
        _texts, tf = dec.decode_batch(None, dev, token_frames=True)
        targets = [tf.label[int(tf.offsets[u]):int(tf.offsets[u + 1])].tolist() for u in range(n)]
        decode_ms = []
        for k in range(args.steps + 1):
            t0 = time.perf_counter()
            dec.decode_batch(None, dev)
            decode_ms.append((time.perf_counter() - t0) * 1e3)
        wall, native, sniff, lse, vit = [], [], [], [], []
        for k in range(args.steps + 1):
            t0 = time.perf_counter()
            out = dec.align_batch(dev, tokens=targets, confidence="mean")
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = dec.last_align_timing_ms
            sniff.append(ms[0]), lse.append(ms[1]), vit.append(ms[2]), native.append(ms[3])
        assert all(a is not None and len(a.path) == T for a in out)
        med = lambda v: float(np.median(v[1:]))  # noqa: E731
        read = n * T * V * 4
        dev_ms = med(sniff) + med(lse) + med(vit)
        lines += [
            "%d utterances (%.0f target tokens on average, %d ctc_viterbi launch(es)):" % (n, np.mean([len(t) for t in targets]),
                                                                                          dec.last_align_launches),
            "  row_lse          %9.3f ms  (%.2f GB read: %.1f %% of the 8 TB/s peak)" % (med(lse), read / 1e9, 100.0 * read / (med(lse) * 1e-3) / HBM_PEAK),
            "  ctc_viterbi      %9.3f ms" % med(vit),
            "  classification   %9.3f ms  (the decode's own frame-prune stage and sniff, at a threshold of 0)" % med(sniff),
            "  native call      %9.3f ms  (host share %.3f ms: validation, staging, result copies)" % (med(native), med(native) - dev_ms),
            "  align_batch      %9.3f ms  (Python share %.3f ms: targets in, AlignedText objects out)" % (med(wall), med(wall) - med(native)),
            "  decode_batch     %9.3f ms  (the plain beam-search step on the same tensor, for scale)" % med(decode_ms),
        ]
        del dev
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
