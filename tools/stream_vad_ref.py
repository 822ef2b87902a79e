"""The literal restatement behind live sessions that cut at pauses: what a VAD session must deliver, stated OFFLINE on the whole
sequence of probabilities.  No incremental state here: the tests hold csrc/wa_stream_vad.h, which is incremental, to these lists.

  segments(probs, params)         whisper_vad_segments_from_probs (whisper.cpp:5202-5436), integer for integer: [(start_cs, end_cs)]
  utterance_range(seg, T)         the samples of a segment on the session's 16 kHz axis: (start, length)
  finish(raw, c, audio_len)       its merge pass, min_speech erase and padding alone, on given speeches of the first pass
  capped(probs, params, cap_ms)   the same list with the length cap's split rule: a merge whose padded result would be a longer utterance than
                                  cap_ms is not made, the close-neighbour padding is applied at that boundary at once; ([(start_cs, end_cs, split)],
                                  number of splits).  Without a split it is `segments`.
  emit_windows(probs, params)     for every segment of `segments`, the window after which no later audio can change it (None: only the end of input
                                  decides it) and the end of its last raw speech

`params`: dict(threshold, min_speech_duration_ms, min_silence_duration_ms, max_speech_duration_s, speech_pad_ms).  Floats are numpy float32
where the reference computes in float."""
import numpy as np

RATE, WINDOW, GAP = 16000, 512, 3200
INT_MAX = 2 ** 31 - 1
DEFAULTS = dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100, max_speech_duration_s=30.0, speech_pad_ms=30)


def cs_to_samples(cs):
    return int((cs / 100.0) * RATE + 0.5)


def samples_to_cs(n):
    return int((n / float(RATE)) * 100.0 + 0.5)


def utterance_range(seg, T):
    start, end = cs_to_samples(seg[0]), min(cs_to_samples(seg[1]), T)
    return start, max(end - start, 0)


def constants(params):
    p = dict(DEFAULTS, **params)
    thr = np.float32(p["threshold"])
    pad = RATE * p["speech_pad_ms"] // 1000
    if np.float32(p["max_speech_duration_s"]) > np.float32(100000.0):
        max_speech = INT_MAX // 2
    else:
        temp = RATE * int(np.float32(p["max_speech_duration_s"])) - WINDOW - 2 * pad
        max_speech = INT_MAX // 2 if temp > INT_MAX else temp
        if max_speech < 0:
            max_speech = INT_MAX // 2
    neg = np.float32(thr - np.float32(0.15))
    if neg < np.float32(0.01):
        neg = np.float32(0.01)
    return dict(thr=thr, neg=neg, min_silence=RATE * p["min_silence_duration_ms"] // 1000, min_speech=RATE * p["min_speech_duration_ms"] // 1000,
                pad=pad, max_speech=max_speech, silence_at_max=RATE * 98 // 1000)


def first_pass(probs, c):
    """the loop over the probabilities: [(start, end, window that pushed it or None for the one behind the loop)] and, per window, whether a
    candidate is open after it and where it began"""
    speeches, state = [], []
    is_speech = has_curr = False
    temp_end = prev_end = next_start = curr_start = 0
    for i, prob in enumerate(np.asarray(probs, np.float32)):
        cur = WINDOW * i
        while True:          # one pass; `break` is the reference's `continue`
            if prob >= c["thr"] and temp_end:
                temp_end = 0
                if next_start < prev_end:
                    next_start = cur
            if prob >= c["thr"] and not is_speech:
                is_speech = has_curr = True
                curr_start = cur
                break
            if is_speech and cur - curr_start > c["max_speech"]:
                if prev_end:
                    speeches.append((curr_start, prev_end, i))
                    has_curr = True
                    if next_start < prev_end:
                        is_speech = has_curr = False
                    else:
                        curr_start = next_start
                    prev_end = next_start = temp_end = 0
                else:
                    speeches.append((curr_start, cur, i))
                    prev_end = next_start = temp_end = 0
                    is_speech = has_curr = False
                    break
            if prob < c["neg"] and is_speech:
                if not temp_end:
                    temp_end = cur
                if cur - temp_end > c["silence_at_max"]:
                    prev_end = temp_end
                if cur - temp_end < c["min_silence"]:
                    break
                if temp_end - curr_start > c["min_speech"]:
                    speeches.append((curr_start, temp_end, i))
                prev_end = next_start = temp_end = 0
                is_speech = has_curr = False
                break
            break
        state.append((is_speech, curr_start))
    audio_len = len(probs) * WINDOW
    if has_curr and audio_len - curr_start > c["min_speech"]:
        speeches.append((curr_start, audio_len, None))
    return speeches, state


def finish(raw, c, audio_len):
    """merge pass, min_speech erase, padding and centiseconds on the first pass's speeches [(start, end)]"""
    speeches = [[s, e] for s, e in raw]
    i = 0
    while i < len(speeches) - 1:          # merge neighbours less than 200 ms apart
        if speeches[i + 1][0] - speeches[i][1] < GAP:
            speeches[i][1] = speeches[i + 1][1]
            del speeches[i + 1]
        else:
            i += 1
    speeches = [s for s in speeches if not s[1] - s[0] < c["min_speech"]]
    pad = c["pad"]
    out = []
    for i, s in enumerate(speeches):
        if i == 0:
            s[0] = s[0] - pad if s[0] > pad else 0
        if i < len(speeches) - 1:
            nxt = speeches[i + 1]
            silence = nxt[0] - s[1]
            if silence < 2 * pad:
                s[1] += silence // 2
                nxt[0] = nxt[0] - silence // 2 if nxt[0] > silence // 2 else 0
            else:
                s[1] = s[1] + pad if s[1] + pad < audio_len else audio_len
                nxt[0] = nxt[0] - pad if nxt[0] > pad else 0
        else:
            s[1] = s[1] + pad if s[1] + pad < audio_len else audio_len
        out.append((samples_to_cs(s[0]), samples_to_cs(s[1])))
    return out


def segments(probs, params):
    c = constants(params)
    return finish([(s, e) for s, e, _ in first_pass(probs, c)[0]], c, len(probs) * WINDOW)


def capped(probs, params, cap_ms, raw=None, audio_len=None):
    c = constants(params)
    pad, cap = c["pad"], cap_ms * (RATE // 1000)
    if raw is None:
        raw, audio_len = [(s, e) for s, e, _ in first_pass(probs, c)[0]], len(probs) * WINDOW
    merged, splits = [], 0                # dict(start, end, start_pad, end_pad, split)
    for s, e in raw:
        start_pad = pad
        if merged and s - merged[-1]["end"] < GAP:
            m = merged[-1]
            joined = (samples_to_cs(m["start"] - m["start_pad"] if m["start"] > m["start_pad"] else 0), samples_to_cs(e + pad))
            if cs_to_samples(joined[1]) - cs_to_samples(joined[0]) <= cap:
                m["end"] = e
                continue
            silence = s - m["end"]
            if silence < 2 * pad:
                m["end_pad"] = start_pad = silence // 2
            m["split"] = True
            splits += 1
        merged.append(dict(start=s, end=e, start_pad=start_pad, end_pad=pad, split=False))
    out = []
    for m in merged:
        if m["end"] - m["start"] < c["min_speech"]:
            continue
        start = m["start"] - m["start_pad"] if m["start"] > m["start_pad"] else 0
        end = m["end"] + m["end_pad"] if m["end"] + m["end_pad"] < audio_len else audio_len
        out.append((samples_to_cs(start), samples_to_cs(end), m["split"]))
    return out, splits


def emit_windows(probs, params):
    """[(window index or None, raw end)] per segment of segments(probs, params) - for inputs where `capped` makes no split.  A merged speech that
    ends at e is decided after the first window i, not before the window that pushed its last raw speech, with 512 (i + 1) - e >= 3200 and no
    candidate open that began less than 3200 behind e; never, if the speech was pushed behind the loop or no such window exists."""
    c = constants(params)
    raw, state = first_pass(probs, c)
    merged = []
    for s, e, w in raw:
        if merged and s - merged[-1][1] < GAP:
            merged[-1][1], merged[-1][2] = e, w
        else:
            merged.append([s, e, w])
    out = []
    for k, (s, e, w) in enumerate(merged):
        at = None
        if w is not None:
            for i in range(w, len(probs)):
                open_, began = state[i]
                if WINDOW * (i + 1) - e >= GAP and (not open_ or began - e >= GAP):
                    at = i
                    break
        if not e - s < c["min_speech"]:
            out.append((at, e))
    return out
