"""Long recordings: a numpy / plain-Python restatement of what whisper_amd_full_long does around the transcription itself - the layout of a
chunk's speech-only audio, its time table, mapping a time back, and the greedy chunk planner (whisper-rust_amd/csrc/wa_long_plan.h,
wa_vad_host.cpp: wa_vad_map_time).  Written from the reference's VAD step (whisper.cpp:6644-6790, 7882-7921), independent of the product's
code: the tests (tests/test_long_*.py) hold the product to it.  Integer arithmetic is Python's, the two float products are rounded as C does."""
import numpy as np

SR = 16000
SILENCE = 1600              # 0.1 s between segments


def cs_to_samples(cs):
    return int((cs / 100.0) * SR + 0.5)


def samples_to_cs(n):
    return int((n / float(SR)) * 100.0 + 0.5)


def overlap_samples(overlap):
    return int(np.float32(overlap) * np.float32(SR))


def layout_length(segs, overlap, n_samples):
    """The length handed to the transcription for `segs` taken as the whole list."""
    if not segs:
        return 0
    ov, total = overlap_samples(overlap), 0
    for i, (s, e) in enumerate(segs):
        end = cs_to_samples(e) + (ov if i < len(segs) - 1 else 0)
        total += min(end, n_samples - 1) - cs_to_samples(s)
    return max(total + (len(segs) - 1) * SILENCE, 0)


def layout(segs, overlap, n_samples):
    """(length, pieces [(dst, src or -1, len)] unclipped, table [(processed cs, original cs)])."""
    total, ov = layout_length(segs, overlap, n_samples), overlap_samples(overlap)
    pieces, table, off = [], [], 0
    for i, (s, e) in enumerate(segs):
        last = i == len(segs) - 1
        a = min(cs_to_samples(s), n_samples - 1)
        b = min(cs_to_samples(e) + (0 if last else ov), n_samples)
        if b - a <= 0:
            continue
        v0, v1 = samples_to_cs(off), samples_to_cs(off + b - a)
        table += [(v0, s), (v1, e)]
        if v1 - v0 > 100:
            for j in range(1, (v1 - v0) // 20):
                t = v0 + 20 * j
                if t < v1:
                    table.append((t, s + ((t - v0) * (e - s)) // (v1 - v0)))
        pieces.append((off, a, b - a))
        off += b - a
        if not last:
            table += [(samples_to_cs(off), e), (samples_to_cs(off + SILENCE), segs[i + 1][0])]
            pieces.append((off, -1, SILENCE))
            off += SILENCE
    seen, out = set(), []
    for p, o in sorted(table, key=lambda x: x[0]):          # stable: the first entry of equal processed times stays
        if p not in seen:
            seen.add(p)
            out.append((p, o))
    return total, pieces, out


def packed_audio(pcm, segs, overlap):
    """The speech-only audio of `segs` taken as the whole list: zeros where no piece writes, pieces cut at the length."""
    total, pieces, _ = layout(segs, overlap, len(pcm))
    out = np.zeros(total, dtype=np.float32)
    for dst, src, n in pieces:
        n = min(n, total - dst)
        if src >= 0 and n > 0:
            out[dst:dst + n] = pcm[src:src + n]
    return out


def map_time(t, table):
    if not table:
        return t
    if t <= table[0][0]:
        return table[0][1]
    if t >= table[-1][0]:
        return table[-1][1]
    k = next(i for i, (p, _) in enumerate(table) if p >= t)
    if table[k][0] == t:
        return table[k][1]
    (p0, o0), (p1, o1) = table[k - 1], table[k]
    return o0 if p1 == p0 else o0 + ((t - p0) * (o1 - o0)) // (p1 - p0)


def plan(segs, n_samples, overlap, cap):
    """Greedy, in order: [(first, count, packed)]; a run takes the next segment while its length stays <= cap."""
    out, first = [], 0
    while first < len(segs):
        count = 1
        while first + count < len(segs) and layout_length(segs[first:first + count + 1], overlap, n_samples) <= cap:
            count += 1
        out.append((first, count, layout_length(segs[first:first + count], overlap, n_samples)))
        first += count
    return out


def map_segments(chunk_results, tables):
    """chunk_results[c] = [(t0, t1, ...)] in chunk-local cs -> [(t0, t1)] in the caller's: mapped, at least 10 cs long, no overlap."""
    out = []
    for res, table in zip(chunk_results, tables):
        for r in res:
            t0, t1 = map_time(r[0], table), map_time(r[1], table)
            if t1 - t0 < 10:
                t1 = t0 + 10
            if out:
                t0 = max(t0, out[-1][1])
            out.append((t0, t1))
    return out
