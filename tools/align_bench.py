"""Times forced alignment (align_batch: row_lse + ctc_viterbi, csrc/ctc_align_hip.hip), transcript likelihood (score_batch:
row_lse + ctc_forward / ctc_forward_wave) and frame posteriors (posteriors_batch with dense=False: row_lse + ctc_posteriors,
next to ctc_forward on the same batch) at the bench shape -- 4096 utterances of 1000 frames x 1024 labels, float32, each
aligned to / scored with its own decoded tokens, and scored with 8 hypotheses (its tokens plus seven copies with one label
substituted), each forward kernel forced in turn -- and at 64 utterances, with the plain decode_batch step of the same process
for scale; then a sweep of target lengths on 256 utterances of random logits, which is what the wave / group threshold of
ctcdec_score_batch rests on. Kernel times are HIP events on the decode stream (ctcdec_alignment_timing, ctcdec_score_batch,
ctcdec_posteriors_timing).
  python tools/align_bench.py [--out profiles/align_bench.txt] [--steps 3] [--legs align,score,posteriors,sweep,gradient,find,gaps,greedy,prefix,prefix_session]
The gradient leg (not in the default set) times gradient_batch -- ctc_grad_rows alone, next to posteriors_batch(dense=False).
The find leg (not in the default set either) times find_batch -- ctc_find / ctc_find_wave forced in turn, alternating: at the
bench shape each utterance searched for 1 and for 8 phrases of 8 labels cut from its own decoded tokens, then 256 and 2048
phrases of 15 / 127 / 511 labels on 256 utterances of random logits, next to ctc_viterbi and ctc_forward on the same batch.
The gaps leg (not in the default set either) times align_gaps_batch next to align_batch on the same batch, alternating:
row_lse_max against row_lse, ctc_viterbi_gaps on the gap-free targets against ctc_viterbi on the same targets, and
ctc_viterbi_gaps again with a leading gap, a trailing gap and one gap at every word boundary.
The greedy leg (not in the default set either) times decode_greedy_batch: row_argmax, row_lse_argmax and greedy_collapse,
next to row_lse_max and decode_batch's frame-prune stage on the same batch in the same rounds, alternating.
The prefix leg (not in the default set either) times prefix_scores_batch with 1, 8 and 16 prefixes of about 20 labels per
utterance -- the first 20 of its decoded tokens, and copies with one label substituted --: ctc_prefix_extend, the forward
kernels with end states next to score_batch's plain ones on the same prefixes in the same rounds, alternating, and row_lse.
The prefix_session leg (not in the default set either) grows a beam of 8 prefixes per utterance to 20 labels in a prefix
session and times steps 1, 10 and 20 -- ctc_prefix_advance, ctc_prefix_extend, the native call -- next to the stateless
prefix_scores_batch on the same prefixes in the same rounds.
The 4096 utterances are 256 distinct ones repeated: no kernel's time depends on the rows being distinct."""
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
PRUNE_RATE = 3.5e12  # bytes / s: what frame_prune reaches on the same logits (README)
_G = {}


def _gen(u):
    g = _G
    return synth.d_words(4, u, T, g["labels"], True, g["words"], g["sentences"], len(g["labels"]), boost=6.0)


def med(v):
    return float(np.median(v[1:]))  # (the first step is the warm-up)


def time_score(dec, dev, hyps, kernel, steps):
    """Medians over `steps` calls after one warm-up of score_batch under CTCDEC_FORWARD_KERNEL=kernel ("" : the library
    chooses): (forward kernels ms, row_lse ms, whole native call ms, Python wall ms, hypotheses per kernel)."""
    if kernel:
        os.environ["CTCDEC_FORWARD_KERNEL"] = kernel
    else:
        os.environ.pop("CTCDEC_FORWARD_KERNEL", None)
    fwd, lse, native, wall = [], [], [], []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        out = dec.score_batch(dev, tokens=hyps)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = dec.last_score_timing_ms
        lse.append(ms[1]), fwd.append(ms[2]), native.append(ms[3])
    os.environ.pop("CTCDEC_FORWARD_KERNEL", None)
    assert all(np.isfinite(g.logp) for per_utt in out for g in per_utt)
    return med(fwd), med(lse), med(native), med(wall), dec.last_score_launched


def score_lines(dec, dev, targets, steps, vit_ms):
    rng = np.random.default_rng(3)
    blank = dec._alphabet.labels.index("")
    pool = [c for c in range(V) if c != blank]
    lines = []
    eight = []
    for t in targets:
        hyps = [list(t)]
        for _ in range(7):
            sub = list(t)
            if sub:
                sub[int(rng.integers(0, len(sub)))] = pool[int(rng.integers(0, len(pool)))]
            hyps.append(sub)
        eight.append(hyps)
    for what, hyps in (("1 hypothesis ", [[t] for t in targets]), ("8 hypotheses", eight)):
        for kernel in ("wave", "group", ""):
            fwd, lse, native, wall, launched = time_score(dec, dev, hyps, kernel, steps)
            lines.append("  score_batch %s %-5s  forward %9.3f ms  row_lse %9.3f ms  native call %9.3f ms  Python call %9.3f ms  "
                         "(wave kernel %d, group kernel %d hypotheses)" % (what, kernel or "auto", fwd, lse, native, wall, launched[0], launched[1]))
            if what.startswith("1") and kernel == "group":
                lines.append("    ctc_forward / ctc_viterbi at this batch: %.2f" % (fwd / vit_ms))
    return lines


def time_posteriors(dec, dev, targets, steps):
    """ctc_posteriors (dense=False) and the group ctc_forward on the same batch, alternating after one warm-up each:
    medians of (posteriors kernel ms, forward kernel ms, posteriors native call ms, posteriors Python call ms), launches."""
    os.environ["CTCDEC_FORWARD_KERNEL"] = "group"
    hyps = [[t] for t in targets]
    post, fwd, native, wall = [], [], [], []
    for _ in range(steps + 1):
        dec.score_batch(dev, tokens=hyps)
        fwd.append(dec.last_score_timing_ms[2])
        t0 = time.perf_counter()
        out = dec.posteriors_batch(dev, tokens=targets, dense=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        post.append(dec.last_posteriors_timing_ms[2]), native.append(dec.last_posteriors_timing_ms[3])
    os.environ.pop("CTCDEC_FORWARD_KERNEL", None)
    assert all(abs(g.logp - g.logp_backward) <= 1e-9 for g in out)
    return med(post), med(fwd), med(native), med(wall), dec.last_posteriors_launches


def posteriors_lines(dec, dev, targets, steps):
    post, fwd, native, wall, launches = time_posteriors(dec, dev, targets, steps)
    table = sum(32 * T * ((2 * len(t) + 1 + 3) // 4) for t in targets)
    return ["  posteriors_batch dense=False  ctc_posteriors %9.3f ms in %d launch(es)  (%.2f GB of tables written and read back)  "
            "native call %9.3f ms  Python call %9.3f ms" % (post, launches, table / 1e9, native, wall),
            "    ctc_posteriors / ctc_forward (%.3f ms, one group-kernel hypothesis each) at this batch: %.2f" % (fwd, post / fwd)]


def gradient_lines(dec, dev, targets, steps):
    """gradient_batch on the device tensor (its rows written in place into one device buffer) and posteriors_batch(dense=False)
    on the same batch, alternating after one warm-up each: ctc_grad_rows alone, the dense ctc_posteriors launches in front of
    it, and the bytes the row kernel must move -- T * (V * (in + out) + 32 * align_chunks(L)) per utterance -- over its time,
    against the rate frame_prune reaches on the same logits."""
    grad, dense, lean, native, wall = [], [], [], [], []
    for _ in range(steps + 1):
        dec.posteriors_batch(dev, tokens=targets, dense=False)
        lean.append(dec.last_posteriors_timing_ms[2])
        t0 = time.perf_counter()
        out = dec.gradient_batch(dev, tokens=targets)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = dec.last_gradient_timing_ms
        dense.append(ms[2]), grad.append(ms[3]), native.append(ms[4])
    assert all(g.grad.is_cuda and g.grad.shape == (T, V) for g in out)
    launches = dec.last_gradient_launches
    del out
    moved = sum(T * (V * (4 + 4) + 32 * ((2 * len(t) + 1 + 3) // 4)) for t in targets)
    rate = moved / (med(grad) * 1e-3)
    return ["  gradient_batch  ctc_grad_rows %9.3f ms  (%.2f GB to move: %.2f TB/s, %.2f of frame_prune's %.1f TB/s)  dense ctc_posteriors "
            "%9.3f ms  (%d launches of both)  native call %9.3f ms  Python call %9.3f ms"
            % (med(grad), moved / 1e9, rate / 1e12, rate / PRUNE_RATE, PRUNE_RATE / 1e12, med(dense), launches, med(native), med(wall)),
            "    ctc_grad_rows / ctc_posteriors dense=False (%.3f ms) at this batch: %.2f" % (med(lean), med(grad) / med(lean))]


def time_find(dec, dev, phrases, kernels, steps):
    """The find kernels' time (HIP events) under each forced kernel, as time_forward measures the forward kernels: one warm-up
    call each, then `steps` alternating rounds. -> {kernel: (median kernel ms, native call ms, Python call ms)}, phrases per kernel"""
    got = {k: [] for k in kernels}
    launched = {}
    for step in range(steps + 1):
        for k in kernels:
            os.environ["CTCDEC_FIND_KERNEL"] = k
            t0 = time.perf_counter()
            out = dec.find_batch(dev, tokens=phrases)
            wall = (time.perf_counter() - t0) * 1e3
            if step:
                got[k].append((dec.last_find_timing_ms[2], dec.last_find_timing_ms[3], wall))
            launched[k] = dec.last_find_launched
    os.environ.pop("CTCDEC_FIND_KERNEL", None)
    assert all(len(g.hits) == 1 for per_utt in out for g in per_utt)
    return {k: tuple(float(np.median([r[i] for r in v])) for i in range(3)) for k, v in got.items()}, launched


def find_lines(dec, dev, targets, steps, phrase_labels=8):
    """Each utterance searched for 1 and for 8 phrases of `phrase_labels` labels cut from its own decoded tokens, the two
    kernels alternating."""
    rng = np.random.default_rng(9)
    cuts = []
    for t in targets:
        cur = []
        for _ in range(8):
            k = int(rng.integers(0, max(1, len(t) - phrase_labels + 1)))
            cur.append(list(t[k:k + phrase_labels]))
        cuts.append(cur)
    lines = []
    for what, phrases in (("1 phrase ", [c[:1] for c in cuts]), ("8 phrases", cuts)):
        got, launched = time_find(dec, dev, phrases, ("wave", "group"), steps)
        for k in ("wave", "group"):
            lines.append("  find_batch %s of %d labels  %-5s  find kernel %9.3f ms  native call %9.3f ms  Python call %9.3f ms  "
                         "(wave kernel %d, group kernel %d phrases)" % ((what, phrase_labels, k) + got[k] + tuple(launched[k])))
    return lines


def find_sweep_lines(dec, steps):
    """256 utterances of standard-normal logits x 3, random phrases without repeats of 15 / 127 / 511 labels, one and eight per
    utterance (256 and 2048 phrases): both find kernels where both take the length, alternating, next to ctc_viterbi and the
    group ctc_forward on the same batch with the same label sequences in the same run."""
    import torch

    lines = ["find: sweep of phrase lengths, 256 utterances x %d frames x %d labels float32 (random logits), 1 and 8 phrases per "
             "utterance; %d alternating steps after one warm-up each, medians (kernels alone, HIP events):" % (T, V, steps),
             "  %6s | %12s %12s %10s | %12s %12s %10s | %12s %12s | %8s %8s" % (
                 "labels", "wave x1", "group x1", "wave/group", "wave x8", "group x8", "wave/group", "ctc_viterbi", "ctc_forward",
                 "find/vit", "find/fwd")]
    rng = np.random.default_rng(5)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    blank = dec._alphabet.labels.index("")
    pool = np.array([c for c in range(V) if c != blank])
    dev = torch.randn((DISTINCT, T, V), generator=gen, device="cuda", dtype=torch.float32) * 3
    torch.cuda.synchronize()
    for L in (15, 127, 511, 15):  # (15 labels twice: what the first row measures may be the first use, not the length)
        ones, eights = [], []
        for _ in range(DISTINCT):
            cur = []
            for _k in range(8):
                t = pool[rng.integers(0, len(pool), size=L)]
                same = np.flatnonzero(t[1:] == t[:-1]) + 1
                t[same] = pool[(np.searchsorted(pool, t[same]) + 1) % len(pool)]
                cur.append(t.tolist())
            ones.append(cur[:1])
            eights.append(cur)
        kernels = ("wave", "group") if L <= 127 else ("group",)
        one = {k: v[0] for k, v in time_find(dec, dev, ones, kernels, steps)[0].items()}
        many = {k: v[0] for k, v in time_find(dec, dev, eights, kernels, steps)[0].items()}
        targets = [c[0] for c in ones]
        fwd = time_forward(dec, dev, ones, ("group",), steps)["group"]
        vit = []
        for _ in range(steps + 1):
            dec.align_batch(dev, tokens=targets)
            vit.append(dec.last_align_timing_ms[2])
        cell = lambda d, k: "%9.3f ms" % d[k] if k in d else "%12s" % "-"  # noqa: E731
        ratio = lambda d: "%10.2f" % (d["wave"] / d["group"]) if "wave" in d else "%10s" % "-"  # noqa: E731
        lines.append("  %6d | %s %s %s | %s %s %s | %9.3f ms %9.3f ms | %8.2f %8.2f" % (
            L, cell(one, "wave"), cell(one, "group"), ratio(one), cell(many, "wave"), cell(many, "group"), ratio(many),
            med(vit), fwd, one["group"] / med(vit), one["group"] / fwd))
    del dev
    return lines


def gaps_lines(dec, dev, targets, steps):
    """align_batch and align_gaps_batch on the same batch, one warm-up round and then `steps` rounds that alternate between
    align, the gap-free targets, a leading gap, a trailing gap and one gap at every word boundary (kernels alone, HIP events on
    the decode stream; medians)."""
    some = next(c for c, lab in enumerate(dec._alphabet.labels) if lab != "")
    targets = [list(t) if len(t) else [some] for t in targets]  # (a target needs a label)

    def between_words(t):
        starts = {lo for _w, lo, _hi in dec._words_of_target(t)[2][1:]}  # (a BPE alphabet: every label is a token)
        out = []
        for k, c in enumerate(t):
            if k in starts:
                out.append(-1)
            out.append(c)
        return out

    forms = [("no gap", targets),
             ("leading gap", [[-1] + list(t) for t in targets]),
             ("trailing gap", [list(t) + [-1] for t in targets]),
             ("gap per word boundary", [between_words(t) for t in targets])]
    n_gaps = float(np.mean([sum(1 for c in t if c == -1) for t in forms[3][1]]))
    lse, vit = [], []
    got = {name: ([], [], [], []) for name, _ in forms}
    for step in range(steps + 1):
        dec.align_batch(dev, tokens=targets)
        ms = dec.last_align_timing_ms
        if step:
            lse.append(ms[1]), vit.append(ms[2])
        for name, items in forms:
            t0 = time.perf_counter()
            out = dec.align_gaps_batch(dev, tokens=items)
            wall = (time.perf_counter() - t0) * 1e3
            ms = dec.last_align_gaps_timing_ms
            if step:
                for k, v in enumerate((ms[1], ms[2], ms[3], wall)):
                    got[name][k].append(v)
            assert all(a is not None and len(a.path) == T for a in out)
    m = lambda v: float(np.median(v))  # noqa: E731
    read = len(targets) * T * V * 4
    lse_max = m([v for name, _ in forms for v in got[name][0]])
    lines = ["  row_lse          %9.3f ms   row_lse_max %9.3f ms  (%.2f of row_lse; %.2f GB read: %.1f %% of the 8 TB/s peak)"
             % (m(lse), lse_max, lse_max / m(lse), read / 1e9, 100.0 * read / (lse_max * 1e-3) / HBM_PEAK),
             "  ctc_viterbi      %9.3f ms   (the same targets, the same run; %.2f us per frame of the launch)"
             % (m(vit), m(vit) * 1e3 / T)]
    for name, _ in forms:
        g = got[name]
        extra = "  (%.1f gaps on average)" % n_gaps if name.startswith("gap per") else ""
        lines.append("  ctc_viterbi_gaps %9.3f ms   %-22s %.2f of ctc_viterbi  native call %9.3f ms  Python call %9.3f ms%s"
                     % (m(g[1]), name, m(g[1]) / m(vit), m(g[2]), m(g[3]), extra))
    return lines


def greedy_lines(dec, dev, targets, n, steps):
    """decode_greedy_batch without and with confidences, align_gaps_batch on the gap-free decoded targets (its row_lse_max is the
    kernel row_lse_argmax adds an index to) and the plain decode_batch step (its frame-prune stage reads the same bytes), one
    warm-up round and then `steps` alternating rounds: kernels alone (HIP events on the decode stream), the native calls and
    the Python calls; medians, and the spread of the rounds for the two log-sum-exp kernels."""
    some = next(c for c, lab in enumerate(dec._alphabet.labels) if lab != "")
    targets = [list(t) if len(t) else [some] for t in targets]  # (align_gaps: a target needs a label)
    got = {k: [] for k in ("argmax", "collapse", "native", "wall", "lse_argmax", "collapse_c", "native_c", "wall_c", "lse_max", "prune")}
    tokens = 0
    for step in range(steps + 1):
        t0 = time.perf_counter()
        texts = dec.decode_greedy_batch(dev)
        wall = (time.perf_counter() - t0) * 1e3
        ms = dec.last_greedy_timing_ms
        assert ms[0] == 0.0 and dec.last_greedy_lse_ms == 0.0 and len(texts) == n
        row = [("argmax", ms[1]), ("collapse", ms[2]), ("native", ms[3]), ("wall", wall)]
        t0 = time.perf_counter()
        _texts, frames = dec.decode_greedy_batch(dev, confidence="mean")
        wall = (time.perf_counter() - t0) * 1e3
        ms = dec.last_greedy_timing_ms
        tokens = int(frames.offsets[-1])
        assert _texts == texts and np.isfinite(frames.score).all()
        row += [("lse_argmax", ms[1]), ("collapse_c", ms[2]), ("native_c", ms[3]), ("wall_c", wall)]
        dec.align_gaps_batch(dev, tokens=targets)
        row.append(("lse_max", dec.last_align_gaps_timing_ms[1]))
        dec.decode_batch(None, dev)
        row.append(("prune", dec.last_timing_ms[0]))
        if step:
            for k, v in row:
                got[k].append(v)
    m = lambda k: float(np.median(got[k]))  # noqa: E731
    spread = lambda k: max(got[k]) - min(got[k])  # noqa: E731
    read = n * T * V * 4
    tbs = lambda ms: read / (ms * 1e-3) / 1e12  # noqa: E731
    return [
        "  greedy decode, %d tokens in all" % tokens,
        "  row_argmax       %9.3f ms  (%.2f GB read: %.2f TB/s; frame_prune reaches %.1f TB/s on the same bytes, the chip streams about 6.3)"
        % (m("argmax"), read / 1e9, tbs(m("argmax")), PRUNE_RATE / 1e12),
        "  greedy_collapse  %9.3f ms  (count pass and write pass)   with confidences %9.3f ms" % (m("collapse"), m("collapse_c")),
        "  decode_greedy_batch                    native call %9.3f ms  Python call %9.3f ms" % (m("native"), m("wall")),
        "  row_lse_argmax   %9.3f ms  (%.2f TB/s)   row_lse_max %9.3f ms in the same rounds  (%.3f of it; spread of the rounds: "
        "row_lse_argmax %.3f ms, row_lse_max %.3f ms)"
        % (m("lse_argmax"), tbs(m("lse_argmax")), m("lse_max"), m("lse_argmax") / m("lse_max"), spread("lse_argmax"), spread("lse_max")),
        "  decode_greedy_batch confidence='mean'  native call %9.3f ms  Python call %9.3f ms" % (m("native_c"), m("wall_c")),
        "  decode_batch's frame-prune stage %9.3f ms in the same rounds  (%.2f TB/s)" % (m("prune"), tbs(m("prune"))),
    ]


def prefix_lines(dec, dev, targets, n, steps):
    rng = np.random.default_rng(11)
    blank = dec._alphabet.labels.index("")
    pool = [c for c in range(V) if c != blank]
    sixteen = []
    for t in targets:
        head = list(t[:20])
        cur = [head]
        for _ in range(15):
            sub = list(head)
            if sub:
                sub[int(rng.integers(0, len(sub)))] = pool[int(rng.integers(0, len(pool)))]
            cur.append(sub)
        sixteen.append(cur)
    read = n * T * V * 4
    lines = ["  prefix scores, prefixes of %.0f labels on average" % np.mean([len(c[0]) for c in sixteen])]
    ext_of = {}
    for per_utt in (1, 8, 16):
        prefixes = [c[:per_utt] for c in sixteen]
        got = {k: [] for k in ("extend", "ends", "lse", "native", "wall", "plain")}
        for step in range(steps + 1):
            t0 = time.perf_counter()
            out = dec.prefix_scores_batch(dev, tokens=prefixes)
            wall = (time.perf_counter() - t0) * 1e3
            ms = dec.last_prefix_timing_ms
            dec.score_batch(dev, tokens=prefixes)
            if step:
                for k, v in (("extend", ms[3]), ("ends", ms[2]), ("lse", ms[1]), ("native", ms[4]), ("wall", wall),
                             ("plain", dec.last_score_timing_ms[2])):
                    got[k].append(v)
        assert all(np.isfinite(g.logp_end) for per in out for g in per)
        del out
        m = lambda k: float(np.median(got[k]))  # noqa: E731
        spread = lambda k: max(got[k]) - min(got[k])  # noqa: E731
        ext_of[per_utt] = m("extend")
        lines.append("  %2d prefix(es) per utterance: ctc_prefix_extend %9.3f ms (spread %.3f; %.2f TB/s of the %.2f GB of logits per chunk "
                     "of 8)  forward with end states %9.3f ms  plain forward (score_batch, same rounds) %9.3f ms  ratio %.3f  (spreads %.3f / %.3f)"
                     % (per_utt, m("extend"), spread("extend"), -(-per_utt // 8) * read / (m("extend") * 1e-3) / 1e12, read / 1e9,
                        m("ends"), m("plain"), m("ends") / m("plain"), spread("ends"), spread("plain")))
        lines.append("      row_lse %9.3f ms  (ctc_prefix_extend / row_lse %.2f)  native call %9.3f ms  Python call %9.3f ms  launches %s"
                     % (m("lse"), m("extend") / m("lse"), m("native"), m("wall"), dec.last_prefix_launches))
    lines.append("    ctc_prefix_extend, 8 prefixes / 1 prefix: %.2f   16 / 8: %.2f" % (ext_of[8] / ext_of[1], ext_of[16] / ext_of[8]))
    return lines


def prefix_session_lines(dec, dev, targets, n, steps, beam=8, depth=20, at=(1, 10, 20)):
    """A beam of `beam` prefixes per utterance grown from the roots to `depth` labels in a prefix session -- beam 0 along the
    utterance's own decoded tokens, the others along random labels; every prefix one label longer per step, the parents
    released --, one warm-up round and then `steps` rounds. At the steps `at`: ctc_prefix_advance, ctc_prefix_extend and the
    native call of the session's extend, and in the same round the stateless prefix_scores_batch on the same prefixes: its
    forward kernels, row_lse, ctc_prefix_extend and native call. The stateless call is the baseline."""
    rng = np.random.default_rng(13)
    blank = dec._alphabet.labels.index("")
    pool = [c for c in range(V) if c != blank]
    paths = [[[int(t[k]) if j == 0 and k < len(t) else pool[int(rng.integers(0, len(pool)))] for k in range(depth)]
              for j in range(beam)] for t in targets]
    keys = ("advance", "s_extend", "s_native", "s_wall", "forward", "lse", "extend", "native", "wall", "open")
    got = {step: {k: [] for k in keys} for step in at}
    launches = {}
    for rnd in range(steps + 1):
        t0 = time.perf_counter()
        s = dec.prefix_session(dev, capacity=n * (1 + 2 * beam))
        opened = (time.perf_counter() - t0) * 1e3
        with s:
            live = [r for r in s.roots for _j in range(beam)]
            for step in range(1, depth + 1):
                t0 = time.perf_counter()
                kids = s.extend([p.id for p in live], [paths[u][j][step - 1] for u in range(n) for j in range(beam)])
                wall = (time.perf_counter() - t0) * 1e3
                ms, launches[step] = s.last_timing_ms, s.last_launches
                if step > 1:
                    s.release([p.id for p in live])
                live = kids
                if step not in at:
                    continue
                row = [("advance", ms[0]), ("s_extend", ms[1]), ("s_native", ms[2]), ("s_wall", wall), ("open", opened)]
                prefixes = [[paths[u][j][:step] for j in range(beam)] for u in range(n)]
                t0 = time.perf_counter()
                out = dec.prefix_scores_batch(dev, tokens=prefixes)
                wall = (time.perf_counter() - t0) * 1e3
                ms = dec.last_prefix_timing_ms
                row += [("forward", ms[2]), ("lse", ms[1]), ("extend", ms[3]), ("native", ms[4]), ("wall", wall)]
                # (the session's bits are the stateless call's: checked here on the first and the last utterance)
                for u in (0, n - 1):
                    for j in range(beam):
                        a, b = kids[u * beam + j], out[u][j]
                        assert a.tokens == b.tokens and a.logp_end == b.logp_end and bool((a.next_logp == b.next_logp).all())
                del out
                if rnd:
                    for k, v in row:
                        got[step][k].append(v)
            del live, kids
        print("prefix session, %d utterances: round %d of %d done" % (n, rnd, steps), file=sys.stderr, flush=True)
    lines = ["  prefix session, a beam of %d prefixes per utterance grown to %d labels; the stateless prefix_scores_batch on the same "
             "prefixes in the same rounds is the baseline (median, spread of the rounds)" % (beam, depth),
             "  open (classification, row_lse, the roots' forward pass and extension, arena): Python call %9.3f ms" % float(np.median(got[at[0]]["open"]))]
    cell = lambda step, k: "%9.3f (%.3f)" % (float(np.median(got[step][k])), max(got[step][k]) - min(got[step][k]))  # noqa: E731
    for step in at:
        lines.append("  step %2d  session:   ctc_prefix_advance %s ms  ctc_prefix_extend %s ms  native call %s ms  Python call %s ms  launches %s"
                     % (step, cell(step, "advance"), cell(step, "s_extend"), cell(step, "s_native"), cell(step, "s_wall"), launches[step]))
        lines.append("           stateless: forward kernels    %s ms  ctc_prefix_extend %s ms  row_lse %s ms  native call %s ms  Python call %s ms"
                     % (cell(step, "forward"), cell(step, "extend"), cell(step, "lse"), cell(step, "native"), cell(step, "wall")))
        lines.append("           native call, stateless / session: %.2f   advance / ctc_prefix_extend: %.2f"
                     % (float(np.median(got[step]["native"])) / float(np.median(got[step]["s_native"])),
                        float(np.median(got[step]["advance"])) / float(np.median(got[step]["s_extend"]))))
    return lines


def time_forward(dec, dev, hyps, kernels, steps):
    """The forward kernels' time (HIP events) under each forced kernel: one warm-up call each, then `steps` rounds that
    alternate between them (clocks as they come: neither kernel gets the warmer half of the run). -> {kernel: median ms}"""
    got = {k: [] for k in kernels}
    for step in range(steps + 1):
        for k in kernels:
            os.environ["CTCDEC_FORWARD_KERNEL"] = k
            dec.score_batch(dev, tokens=hyps)
            if step:
                got[k].append(dec.last_score_timing_ms[2])
    os.environ.pop("CTCDEC_FORWARD_KERNEL", None)
    return {k: float(np.median(v)) for k, v in got.items()}


def sweep_lines(dec, steps):
    """256 utterances of standard-normal logits x 3, random targets without repeats of each length, one hypothesis and eight
    (the target plus seven copies with one label substituted) per utterance: both forward kernels where both take the length,
    and ctc_viterbi on the same batch."""
    import torch

    lines = ["sweep of target lengths, 256 utterances x %d labels float32 (random logits), 1 and 8 hypotheses per utterance; "
             "%d alternating steps after one warm-up each, medians:" % (V, steps),
             "  %6s %6s | %12s %12s %10s | %12s %12s %10s | %12s %8s" % (
                 "labels", "frames", "wave x1", "group x1", "wave/group", "wave x8", "group x8", "wave/group", "ctc_viterbi", "fwd/vit")
             + " | %14s %8s" % ("ctc_posteriors", "post/fwd")]
    rng = np.random.default_rng(5)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    blank = dec._alphabet.labels.index("")
    pool = np.array([c for c in range(V) if c != blank])
    # (15 labels twice, first and last: what the first row of a sweep measures may be the first use, not the length)
    for L in (15, 31, 63, 127, 255, 511, 2047, 15):
        frames = T if L < T - 100 else 2100
        dev = torch.randn((DISTINCT, frames, V), generator=gen, device="cuda", dtype=torch.float32) * 3
        torch.cuda.synchronize()
        targets, eight = [], []
        for _ in range(DISTINCT):
            t = pool[rng.integers(0, len(pool), size=L)]
            same = np.flatnonzero(t[1:] == t[:-1]) + 1
            t[same] = pool[(np.searchsorted(pool, t[same]) + 1) % len(pool)]
            targets.append(t.tolist())
            hyps = [t.tolist()]
            for _k in range(7):
                sub = t.copy()
                sub[int(rng.integers(0, L))] = pool[int(rng.integers(0, len(pool)))]
                hyps.append(sub.tolist())
            eight.append(hyps)
        kernels = ("wave", "group") if L <= 127 else ("group",)
        one = time_forward(dec, dev, [[t] for t in targets], kernels, steps)
        many = time_forward(dec, dev, eight, kernels, steps)
        vit = []
        for _ in range(steps + 1):
            dec.align_batch(dev, tokens=targets)
            vit.append(dec.last_align_timing_ms[2])
        cell = lambda d, k: "%9.3f ms" % d[k] if k in d else "%12s" % "-"  # noqa: E731
        ratio = lambda d: "%10.2f" % (d["wave"] / d["group"]) if "wave" in d else "%10s" % "-"  # noqa: E731
        post, fwd = time_posteriors(dec, dev, targets, steps)[:2]
        lines.append("  %6d %6d | %s %s %s | %s %s %s | %9.3f ms %8.2f | %11.3f ms %8.2f" % (
            L, frames, cell(one, "wave"), cell(one, "group"), ratio(one), cell(many, "wave"), cell(many, "group"), ratio(many),
            med(vit), one["group"] / med(vit), post, post / fwd))
        del dev
    return lines


def align_lines(dec, dev, targets, n, steps):
    """-> (ctc_viterbi ms, lines): align_batch with confidences, and the plain decode_batch step for scale."""
    decode_ms = []
    for k in range(steps + 1):
        t0 = time.perf_counter()
        dec.decode_batch(None, dev)
        decode_ms.append((time.perf_counter() - t0) * 1e3)
    wall, native, sniff, lse, vit = [], [], [], [], []
    for k in range(steps + 1):
        t0 = time.perf_counter()
        out = dec.align_batch(dev, tokens=targets, confidence="mean")
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = dec.last_align_timing_ms
        sniff.append(ms[0]), lse.append(ms[1]), vit.append(ms[2]), native.append(ms[3])
    assert all(a is not None and len(a.path) == T for a in out)
    read = n * T * V * 4
    dev_ms = med(sniff) + med(lse) + med(vit)
    lines = [
        "  %d ctc_viterbi launch(es)" % dec.last_align_launches,
        "  row_lse          %9.3f ms  (%.2f GB read: %.1f %% of the 8 TB/s peak)" % (med(lse), read / 1e9, 100.0 * read / (med(lse) * 1e-3) / HBM_PEAK),
        "  ctc_viterbi      %9.3f ms" % med(vit),
        "  classification   %9.3f ms  (the decode's own frame-prune stage and sniff, at a threshold of 0)" % med(sniff),
        "  native call      %9.3f ms  (host share %.3f ms: validation, staging, result copies)" % (med(native), med(native) - dev_ms),
        "  align_batch      %9.3f ms  (Python share %.3f ms: targets in, AlignedText objects out)" % (med(wall), med(wall) - med(native)),
        "  decode_batch     %9.3f ms  (the plain beam-search step on the same tensor, for scale)" % med(decode_ms),
    ]
    return med(vit), lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--legs", default="align,score,posteriors,sweep", help="which parts to run (a partial run wants its own --out)")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
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
    lines = ["forced alignment and transcript likelihood, %d frames x %d labels float32 per utterance, targets = the utterance's own decoded tokens; "
             "%d steps after one warm-up, medians" % (T, V, args.steps)]
    for n in (4096, 64):
        dev = base_dev.repeat(n // DISTINCT, 1, 1) if n > DISTINCT else base_dev[:n].contiguous()
        torch.cuda.synchronize()
        _texts, tf = dec.decode_batch(None, dev, token_frames=True)
        targets = [tf.label[int(tf.offsets[u]):int(tf.offsets[u + 1])].tolist() for u in range(n)]
        lines.append("%d utterances (%.0f target tokens on average):" % (n, np.mean([len(t) for t in targets])))
        vit_ms = None
        if "align" in legs:
            vit_ms, align = align_lines(dec, dev, targets, n, args.steps)
            lines += align
        if "score" in legs and vit_ms is not None:
            lines += score_lines(dec, dev, targets, args.steps, vit_ms)
        if "posteriors" in legs:
            lines += posteriors_lines(dec, dev, targets, args.steps)
        if "gradient" in legs:
            lines += gradient_lines(dec, dev, targets, args.steps)
        if "find" in legs:
            lines += find_lines(dec, dev, targets, args.steps)
        if "gaps" in legs:
            lines += gaps_lines(dec, dev, targets, args.steps)
        if "greedy" in legs:
            lines += greedy_lines(dec, dev, targets, n, args.steps)
        if "prefix" in legs:
            lines += prefix_lines(dec, dev, targets, n, args.steps)
        if "prefix_session" in legs:
            lines += prefix_session_lines(dec, dev, targets, n, args.steps)
        del dev
    if "sweep" in legs:
        lines += sweep_lines(dec, max(args.steps, 5))
    if "find" in legs:
        lines += find_sweep_lines(dec, args.steps)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
