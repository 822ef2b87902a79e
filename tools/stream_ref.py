"""The literal restatement of the step mode of the reference's examples/stream/stream.cpp: its vectors pcmf32, pcmf32_old, prompt_tokens and its
counter n_iter, statement for statement, in numpy.  No engine: the caller runs whisper_full on `pcmf32` with `prompt_tokens` and hands the
result's token ids back.  The yardstick of tests/test_stream_plan_math.py and tests/test_stream_full_gpu.py, and the driver of
tools/gen_golden_stream.py.

    ref = StreamRef(step_ms, length_ms, keep_ms)
    for new in ref.steps(audio):              # n_samples_step new samples each
        pcm = ref.window(new)                 # pcmf32 of this iteration
        ids = run(pcm, list(ref.prompt_tokens))
        ref.after(ids)                        # ++n_iter; the new-line rule
"""
import numpy as np

WHISPER_SAMPLE_RATE = 16000


class StreamRef:
    def __init__(self, step_ms: int, length_ms: int, keep_ms: int, no_context: bool = False):
        keep_ms = min(keep_ms, step_ms)
        length_ms = max(length_ms, step_ms)
        self.n_samples_step = int((1e-3 * step_ms) * WHISPER_SAMPLE_RATE)
        self.n_samples_len = int((1e-3 * length_ms) * WHISPER_SAMPLE_RATE)
        self.n_samples_keep = int((1e-3 * keep_ms) * WHISPER_SAMPLE_RATE)
        self.n_new_line = max(1, length_ms // step_ms - 1)
        self.no_context = no_context
        self.pcmf32 = np.zeros(0, np.float32)
        self.pcmf32_old = np.zeros(0, np.float32)
        self.prompt_tokens = []
        self.n_iter = 0
        self.n_samples_take = 0

    def steps(self, audio):
        audio = np.asarray(audio, np.float32)
        for k in range(len(audio) // self.n_samples_step):
            yield audio[k * self.n_samples_step:(k + 1) * self.n_samples_step]

    def window(self, pcmf32_new) -> np.ndarray:
        pcmf32_new = np.asarray(pcmf32_new, np.float32)
        n_samples_new = len(pcmf32_new)
        # take up to params.length_ms audio from previous iteration
        n_samples_take = min(len(self.pcmf32_old), max(0, self.n_samples_keep + self.n_samples_len - n_samples_new))
        pcmf32 = np.zeros(n_samples_new + n_samples_take, np.float32)
        pcmf32[:n_samples_take] = self.pcmf32_old[len(self.pcmf32_old) - n_samples_take:]     # pcmf32[i] = pcmf32_old[size - take + i]
        pcmf32[n_samples_take:] = pcmf32_new
        self.pcmf32 = pcmf32
        self.pcmf32_old = pcmf32.copy()
        self.n_samples_take = n_samples_take
        return pcmf32

    def after(self, token_ids) -> bool:
        """`token_ids`: whisper_full_get_token_id over every segment of the window's result.  True: the line was committed."""
        self.n_iter += 1
        if self.n_iter % self.n_new_line == 0:
            # keep part of the audio for next iteration to try to mitigate word boundary issues
            self.pcmf32_old = self.pcmf32[len(self.pcmf32) - self.n_samples_keep:].copy()
            # Add tokens of the last full length segment as the prompt
            if not self.no_context:
                self.prompt_tokens = [int(t) for t in token_ids]
            return True
        return False


def drive(ref: "StreamRef", audio, run):
    """Every whole step of `audio` through `ref`; `run(pcmf32, prompt_tokens)` returns the window's segments as dicts with "ids".
    Returns one record per window: the window, the prompt it ran with, its segments, whether it committed."""
    out = []
    for new in ref.steps(audio):
        pcm = ref.window(new)
        prompt = list(ref.prompt_tokens)
        segs = run(pcm, prompt)
        out.append(dict(pcm=pcm, take=ref.n_samples_take, prompt=prompt, segs=segs, committed=ref.after([i for s in segs for i in s["ids"]])))
    return out
