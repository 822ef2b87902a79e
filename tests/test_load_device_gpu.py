"""The model loader's two paths through the C ABI: the device path (pinned chunks up, unpack kernels of wa_load.hip write the arena) against the
host path (WHISPER_AMD_LOAD_HOST=1: a host image unpacked by the host functions, one upload).

  * The weight arena (whisper_amd_arena_read) must be the same size and the same bytes after both, for an F16 model, every quantised format,
    a width whose block count is no multiple of 4 (s192), `tiny` (tensors of several chunks), and chunks of ONE row (WHISPER_AMD_LOAD_CHUNK=1:
    the loader raises it to the longest row of the model).  whisper_amd_load_stats names the path taken and the tensor bytes read.
  * The same through the buffer entry point and through a caller's whisper_model_loader - one that serves every read whole, and one whose
    read returns at most 4099 bytes a call: neither path loops on a short read, so both must end the same way, whatever that is.
  * A file cut inside a tensor, exactly at a chunk boundary, and between two tensor records: null from both paths with the same error lines,
    and a good load right after.
  * Greedy full() after a device-path load against the committed goldens of the reference engine.
Everything is equality of bytes, of log lines or of token lists."""
import contextlib
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def load_env(host=False, chunk=None):
    """the loader reads both variables every time a context is created"""
    keys = ("WHISPER_AMD_LOAD_HOST", "WHISPER_AMD_LOAD_CHUNK")
    old = {k: os.environ.pop(k, None) for k in keys}
    if host:
        os.environ["WHISPER_AMD_LOAD_HOST"] = "1"
    if chunk is not None:
        os.environ["WHISPER_AMD_LOAD_CHUNK"] = str(chunk)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def model_file(name):
    return wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)


def tensor_records(data):
    """[(name, first data byte, data bytes, bytes of one row as the loader counts rows, ggml type)] of a legacy-ggml file"""
    at = 4 + 11 * 4
    n_mel, n_fft = struct.unpack_from("<2i", data, at); at += 8 + 4 * n_mel * n_fft
    (n_vocab,) = struct.unpack_from("<i", data, at); at += 4
    for _ in range(n_vocab):
        (ln,) = struct.unpack_from("<I", data, at); at += 4 + ln
    block = {0: (1, 4), 1: (1, 2), 6: (32, 22), 8: (32, 34), 3: (32, 20), 7: (32, 24), 10: (256, 84), 11: (256, 110), 13: (256, 176), 14: (256, 210)}
    out = []
    while at < len(data):
        n_dims, ln, ttype = struct.unpack_from("<3i", data, at); at += 12
        ne = struct.unpack_from("<%di" % n_dims, data, at); at += 4 * n_dims
        name = data[at:at + ln].decode(); at += ln
        per, size = block[ttype]
        nbytes = int(np.prod(ne)) // per * size
        row = ne[0] * ne[1] * size if n_dims == 3 else ne[0] // per * size          # a conv weight's row is one output channel, [ic][3]
        out.append((name, at, nbytes, row, ttype))
        at += nbytes
    assert at == len(data)
    return out


def chunks_of(recs, chunk):
    """[(record index, first byte in the file, bytes)] as the device path cuts the tensors for WHISPER_AMD_LOAD_CHUNK = chunk: buffers of
    the chunk size raised to the longest row and to a multiple of 16, filled tensor after tensor in whole rows, each chunk starting at a
    multiple of 16 (wa_load_plan.h and the loader's one rule: a chunk that does not fit behind the bytes already placed starts a new
    buffer).  The launch count the loader reports holds this restatement to the loader."""
    cap = -(-max(chunk, max(r[3] for r in recs)) // 16) * 16
    used, out = 0, []
    for i, (_, off, nbytes, row, _) in enumerate(recs):
        n_rows, at = nbytes // row, 0
        fit = (cap - used) // row or cap // row
        while at < n_rows:
            rows = min(n_rows - at, fit)
            if used + rows * row > cap:
                used = 0
            out.append((i, off + at * row, rows * row))
            used = -(-(used + rows * row) // 16) * 16
            at, fit = at + rows, cap // row
    return out


def unpacked(rec):
    return rec[4] not in (0, 1) or rec[0] in ("encoder.conv1.weight", "encoder.conv2.weight")


def load(wrs, lib, how, source, host, chunk=None):
    """a context (or None when the library returns null) and the ERROR lines it logged on the way"""
    errors = []
    wrs.set_log_callback(lib, lambda lvl, txt: errors.append(txt) if lvl == 4 else None)
    params = wrs.WhisperContextParameters(lib)
    try:
        with load_env(host, chunk):
            if how == "file":
                ptr = lib.whisper_init_from_file_with_params_no_state(source.encode(), params.c)
            elif how == "buffer":
                arr = np.frombuffer(source, dtype=np.uint8)
                ptr = lib.whisper_init_from_buffer_with_params_no_state(C.c_void_p(arr.ctypes.data), arr.size, params.c)
            else:
                data, max_read, pos = source[0], source[1], [0]

                def rd(_c, out, n):
                    k = min(n, len(data) - pos[0], max_read or n)
                    C.memmove(out, data[pos[0]:pos[0] + k], k)
                    pos[0] += k
                    return k

                loader = wrs.whisper_model_loader(None, wrs.LOADER_READ(rd), wrs.LOADER_EOF(lambda _c: pos[0] >= len(data)), wrs.LOADER_CLOSE(lambda _c: None))
                f = lib.whisper_init_with_params_no_state
                f.restype, f.argtypes = C.c_void_p, [C.POINTER(wrs.whisper_model_loader), wrs.whisper_context_params]
                ptr = f(C.byref(loader), params.c)
    finally:
        wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)          # what the amd_lib fixture installs
    if not ptr:
        return None, errors
    ctx = wrs.WhisperContext(lib, ptr)
    ctx._params = params
    return ctx, errors


def both_ways(wrs, lib, how, source, chunk=None):
    """host path, then device path: (stats, arena) of each, None for a load that returned null; and the error lines of each"""
    out, logs = [], []
    for host in (True, False):
        ctx, errors = load(wrs, lib, how, source, host, chunk)
        logs.append(errors)
        if ctx is None:
            out.append(None)
            continue
        out.append((ctx.load_stats(), ctx.arena()))
        ctx.free()
    return out, logs


def assert_same_arena(got, tensor_bytes, what):
    (hs, ha), (ds, da) = got
    assert hs["path"] == 0 and ds["path"] == 1, (what, hs, ds)
    assert ds["bytes_read"] == tensor_bytes and hs["bytes_read"] == tensor_bytes, (what, hs, ds, tensor_bytes)
    assert hs["kernels"] == 0 and ds["kernels"] >= 2, (what, hs, ds)          # the two conv weights at the least
    assert ha.size == da.size and ha.size > tensor_bytes // 2
    bad = np.flatnonzero(ha != da)
    assert bad.size == 0, "%s: %d of %d arena bytes differ, first at %d" % (what, bad.size, ha.size, bad[0])


# `tiny` at 4 MB: its token embedding (40 MB) and its 2.4 MB matrices then span or share chunks whatever the built-in chunk size is
@pytest.mark.parametrize("name,chunk", [("s128", None), ("s128:q5_0", None), ("s128:q8_0", None), ("s128:q5_1", None), ("s128:q4_1", None),
                                        ("s192:q5_1", None), ("s256:q2_k", None), ("s256:q3_k", None), ("s256:q5_k", None), ("s256:q6_k", None),
                                        ("tiny", None), ("tiny", 4 << 20), ("s128:q5_0", 1), ("s256:q3_k", 1)])
def test_arena_is_the_same_from_both_paths(wrs, amd_lib, name, chunk):
    mp = model_file(name)
    data = open(mp, "rb").read()
    tensor_bytes = sum(r[2] for r in tensor_records(data))
    got, logs = both_ways(wrs, amd_lib, "file", mp, chunk)
    assert got[0] is not None and got[1] is not None and logs == [[], []], logs
    assert_same_arena(got, tensor_bytes, "%s chunk %s" % (name, chunk))
    if ":" in name:
        n_quant = sum(1 for r in tensor_records(data) if r[4] not in (0, 1))
        assert n_quant > 20
        assert got[1][0]["kernels"] >= n_quant + 2
    if chunk is not None:          # one launch per chunk of a quantised or conv tensor: at one row's capacity far more launches than tensors
        recs = tensor_records(data)
        want = sum(1 for i, _, _ in chunks_of(recs, chunk) if unpacked(recs[i]))
        assert got[1][0]["kernels"] == want, (got[1][0], want)
        assert chunk != 1 or want > 3 * len(recs)


def test_buffer_entry_point(wrs, amd_lib):
    data = open(model_file("s128:q5_1"), "rb").read()
    got, logs = both_ways(wrs, amd_lib, "buffer", data)
    assert got[0] is not None and got[1] is not None and logs == [[], []], logs
    assert_same_arena(got, sum(r[2] for r in tensor_records(data)), "buffer")
    file_got, _ = both_ways(wrs, amd_lib, "file", model_file("s128:q5_1"))
    assert np.array_equal(file_got[1][1], got[1][1])


@pytest.mark.parametrize("max_read", [None, 4099])
def test_callers_own_loader(wrs, amd_lib, max_read):
    """max_read None: every read served whole - both paths load, same arena.  4099: reads come back short; the loader loops on none of them,
    in either path, so both must end alike - null with the same error lines, or loaded with the same arena."""
    data = open(model_file("s128:q5_1"), "rb").read()
    got, logs = both_ways(wrs, amd_lib, "loader", (data, max_read))
    assert (got[0] is None) == (got[1] is None), logs
    assert logs[0] == logs[1], logs
    if max_read is None:
        assert got[0] is not None and logs == [[], []]
    if got[0] is not None:
        assert_same_arena(got, sum(r[2] for r in tensor_records(data)), "loader max_read %s" % max_read)
    else:
        assert logs[0], "a refused load says why"


@pytest.mark.parametrize("name", ["s128:q5_0", "s256:q6_k"])
def test_cut_files_fail_alike_and_a_good_load_follows(wrs, amd_lib, tmp_path, name):
    mp = model_file(name)
    data = open(mp, "rb").read()
    recs = tensor_records(data)
    by_name = {r[0]: r for r in recs}
    emb, conv2 = by_name["decoder.token_embedding.weight"], by_name["encoder.conv2.weight"]
    # chunk = 1 byte: the loader raises it to the longest row of the model; a chunk of conv2 that starts inside the tensor
    i_conv2 = recs.index(conv2)
    inner = [c for c in chunks_of(recs, 1) if c[0] == i_conv2 and c[1] > conv2[1]]
    assert len(inner) > 10
    boundary = inner[len(inner) // 2][1]
    cuts = {
        "inside a tensor":          (emb[1] + emb[2] // 2 + 3, None, "truncated tensor 'decoder.token_embedding.weight'"),
        "inside a tensor, 1 row":   (emb[1] + emb[2] // 2 + 3, 1, "truncated tensor 'decoder.token_embedding.weight'"),
        "at a chunk boundary":      (boundary, 1, "truncated tensor 'encoder.conv2.weight'"),
        "between two records":      (recs[len(recs) // 2][1] + recs[len(recs) // 2][2], None, "not all tensors loaded"),
        "between two records, 1 row": (recs[7][1] + recs[7][2], 1, "not all tensors loaded"),
    }
    for what, (size, chunk, expect) in cuts.items():
        p = str(tmp_path / "cut.bin")
        with open(p, "wb") as f:
            f.write(data[:size])
        got, logs = both_ways(wrs, amd_lib, "file", p, chunk)
        assert got == [None, None], what
        assert logs[0] == logs[1] and any(expect in ln for ln in logs[0]), (what, logs)
        assert any("failed to load model" in ln for ln in logs[0]), (what, logs)
    good, logs = both_ways(wrs, amd_lib, "file", mp)
    assert good[0] is not None and good[1] is not None and logs == [[], []]
    assert np.array_equal(good[0][1], good[1][1])


@pytest.mark.parametrize("name,gold_file", [("s128:q5_1", "s128_quant1.json"), ("s256:q5_k", "s256_kquant.json")])
def test_greedy_after_a_device_path_load(wrs, amd_lib, name, gold_file):
    gold = json.load(open(os.path.join(GOLDEN, gold_file)))[name.split(":")[1]]["full"]["greedy_seed0"]
    ctx, errors = load(wrs, amd_lib, "file", model_file(name), host=False)
    assert ctx is not None and not errors
    assert ctx.load_stats()["path"] == 1
    st = ctx.create_state()
    st.full(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0), wsynth.synth_audio(480000, 0))
    got = [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]
    assert got == gold
    st.free()
    ctx.free()


def test_stats_stages_add_up(wrs, amd_lib):
    ctx, _ = load(wrs, amd_lib, "file", model_file("s128:q5_0"), host=False)
    s = ctx.load_stats()
    ctx.free()
    assert s["read_us"] >= 0 and s["wait_us"] >= 0 and s["read_us"] + s["wait_us"] <= s["load_us"], s
