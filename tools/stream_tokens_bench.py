"""Streaming token frames and confidences on the bench's `streaming_cfg5` shape (64 device-resident streams x 50-frame chunks,
V=1024, 4-gram + the bench's hot words, beam 200, device float32 logits): what a chunk costs without the flags, with
token_frames=True and with confidence="mean"; the times of the two ledger kernels (surv_ledger_append per push,
token_logp_ledger per read) from HIP events; and bench.py's own `streaming_cfg5` measurement (bench.extra_streaming, called as
bench.py calls it) five times, for the comparison against the parent commit.

The comparison needs the parent built in a tree of its own and run in the same GPU visit, one process per tree (one library
per process):
  python tools/stream_tokens_bench.py --root <parent tree> --json parent.json      # bench.extra_streaming only
  python tools/stream_tokens_bench.py --parent parent.json [--out profiles/stream_tokens_bench.txt] [--runs 5]"""
import argparse
import inspect
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STREAMS, CHUNK, BEAM = 64, 50, 200


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


def _streams(dec, chunks, scorer, extra, read_at=None):
    """One pass over the chunks -> (ms per unread push, ms of the last push with its results, ms of beams[0] at read_at)"""
    n = N_STREAMS
    states = [dec.get_starting_state() for _ in range(n)]
    beams = [s[0] for s in states]
    push, last, read = [], 0.0, 0.0
    for k, chunk in enumerate(chunks):
        end = k == len(chunks) - 1
        t0 = time.perf_counter()
        beams = dec.partial_decode_beams_batch(chunk, [s[1] for s in states], [s[2] for s in states], beams, [k * CHUNK] * n,
                                               beam_width=BEAM, hotword_scorer=scorer, prune_history=True, is_end=end, **extra)
        dt = 1e3 * (time.perf_counter() - t0)
        if end:
            last = dt
        else:
            push.append(dt)
        if read_at is not None and k == read_at:
            t0 = time.perf_counter()
            _ = [b[0].text for b in beams]
            read = 1e3 * (time.perf_counter() - t0)
    return push, last, read, beams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--root", default=ROOT, help="the tree whose pyctcdecode_amd is measured (default: this one)")
    ap.add_argument("--json", default=None, help="write the bench.extra_streaming figures here (what --parent reads)")
    ap.add_argument("--parent", default=None, help="the --json file of the parent commit's run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_tokens_bench.txt"))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch

    import bench  # (the workload's assets and batch, unchanged)
    from pyctcdecode_amd import build as build_mod
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.language_model import HotwordScorer

    assert os.path.dirname(os.path.abspath(bench.__file__)) == root, bench.__file__
    cache = os.path.join(ROOT, "bench_cache") if os.access(ROOT, os.W_OK) else "/tmp/ctc_bench"
    lm, labels, hot = bench.build_assets(cache, 20000, 60000)
    xs = bench.make_batch(lm, labels, 0, N_STREAMS, bench.T, 6.0, 16)
    dev = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    dec = build_ctcdecoder(labels, lm.path)
    # bench.py's own streaming_cfg5 line, as bench.py produces it
    cfg5 = []
    for _ in range(args.runs):
        line = bench.extra_streaming(torch, dec, dev, bench.T, hot)
        cfg5.append(round(float(line["ms_per_chunk"]), 4))
        print("streaming_cfg5 ms_per_chunk", cfg5[-1], flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"root": root, "runs": args.runs, "ms_per_chunk": cfg5}, f, indent=1)
    if "confidence" not in inspect.signature(dec.partial_decode_beams_batch).parameters:
        return
    n_chunks = bench.T // CHUNK
    chunks = [dev[:, k * CHUNK:(k + 1) * CHUNK].contiguous() for k in range(n_chunks)]
    scorer = HotwordScorer.build_scorer(hot, weight=10.0)
    legs = {"plain": {}, "token_frames": {"token_frames": True}, "confidence": {"confidence": "mean"}}
    res, ends = {}, {}
    for name, extra in legs.items():
        _streams(dec, chunks, scorer, extra)  # (warms the workspaces up)
        push, last, read, ends[name] = _streams(dec, chunks, scorer, extra, read_at=n_chunks // 2)
        res[name] = {"push": float(np.median(push)), "push_min": min(push), "push_max": max(push), "last": last, "best_read": read}
        print(name, json.dumps(res[name]), flush=True)
    # the kernels' own times (HIP events; CTCDEC_HOST_TIMING waits for them, so this pass is not the one that is timed above)
    host = _host_lines(lambda: _streams(dec, chunks, scorer, legs["confidence"], read_at=n_chunks // 2))
    grab = lambda pat: [float(m.group(1)) for ln in host for m in [re.search(pat, ln)] if m]  # noqa: E731
    append_ms = grab(r"surv_ledger_append kernel ([\d.]+) ms")
    ledger_bytes = [int(m.group(1)) for ln in host for m in [re.search(r"(\d+) bytes reserved", ln)] if m]
    fold_ms = grab(r"token_logp_ledger kernel ([\d.]+) ms")
    fold_tokens = [int(m.group(1)) for ln in host for m in [re.search(r"stream token confidences: (\d+) tokens", ln)] if m]
    beam_ms = grab(r"stream push: .*beam kernel ([\d.]+)\)")
    prune_ms = grab(r"stream push: .*\(prune kernel ([\d.]+),")
    plain_key = lambda b: (b.text, list(b.text_frames), b.logit_score, b.lm_score)  # noqa: E731
    same = all([plain_key(b) for b in ends["plain"][u]] == [plain_key(b) for b in ends["confidence"][u]] for u in range(N_STREAMS))
    lines = [
        "Streaming token frames and confidences on the streaming_cfg5 shape: %d streams x %d-frame chunks (%d chunks), V=%d, beam %d, "
        "4-gram + %d hot words, device float32 logits (tools/stream_tokens_bench.py)." % (
            N_STREAMS, CHUNK, n_chunks, bench.V, BEAM, len(hot)),
        "The binary is the one built from the committed sources: pyctcdecode_amd.build.source_tag() = %s, library stamp matches: %s." % (
            build_mod.source_tag()[:16], build_mod._lib_stamp_ok()),
        "",
        "ms per chunk (one push of all %d streams, lists handed back unread), median (min .. max) over %d pushes of one pass after a "
        "warm-up pass; `last` = the is_end push with its results, `best read` = beams[0] of every stream after chunk %d:" % (
            N_STREAMS, n_chunks - 1, n_chunks // 2 + 1),
        "%-14s %10s %22s %12s %12s" % ("leg", "push", "(min .. max)", "last", "best read"),
    ]
    for name in legs:
        r = res[name]
        lines.append("%-14s %10.3f %22s %12.3f %12.3f" % (name, r["push"], "(%.3f .. %.3f)" % (r["push_min"], r["push_max"]), r["last"],
                                                          r["best_read"]))
    lines += [
        "",
        "confidence / plain push: %.4f; token_frames / plain push: %.4f" % (res["confidence"]["push"] / res["plain"]["push"],
                                                                          res["token_frames"]["push"] / res["plain"]["push"]),
        "end results of the confidence streams equal the plain streams' (text, frames, scores): %s" % same,
        "",
        "kernels of one confidence pass, HIP events (a separate pass with CTCDEC_HOST_TIMING=1):",
        "  surv_ledger_append: median %.4f ms per push (min %.4f, max %.4f, %d pushes); the push's prune stage %.3f ms, its beam stage "
        "%.3f ms" % (float(np.median(append_ms)), min(append_ms), max(append_ms), len(append_ms), float(np.median(prune_ms)),
                     float(np.median(beam_ms))),
        "  append / beam stage of the chunk: %.4f%s" % (
            float(np.median(append_ms)) / float(np.median(beam_ms)),
            "" if np.median(append_ms) <= np.median(beam_ms) else "  (ABOVE the beam stage)"),
        "  token_logp_ledger: " + ", ".join("%.4f ms for %d tokens" % (m, t) for m, t in zip(fold_ms, fold_tokens)),
        "  ledger reserved at the end of the streams: %d bytes for %d streams x %d frames (%.1f bytes per frame and stream; the strided "
        "survivor arrays hold max_surv x 10 bytes per frame)" % (ledger_bytes[-1], N_STREAMS, bench.T,
                                                                  ledger_bytes[-1] / (N_STREAMS * bench.T)),
        "",
        "bench.py's streaming_cfg5 measurement (bench.extra_streaming: no flags), ms_per_chunk of %d runs in one process:" % args.runs,
        "  this tree: %s  median %.4f" % (cfg5, float(np.median(cfg5))),
    ]
    if args.parent:
        with open(args.parent) as f:
            parent = json.load(f)
        pm = parent["ms_per_chunk"]
        spread = max(pm) - min(pm)
        diff = float(np.median(cfg5)) - float(np.median(pm))
        lines += [
            "  parent:    %s  median %.4f, run-to-run spread (max - min) %.4f" % (pm, float(np.median(pm)), spread),
            "  this tree - parent (medians): %+.4f ms; within the parent's own spread: %s" % (diff, "yes" if abs(diff) <= spread else "NO"),
            "  (both built from their sources and run in the same GPU visit, one process per tree)",
        ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
