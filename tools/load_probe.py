"""Model load time (wa_model_load): wall time of whisper_init_from_file_with_params_no_state and the loader's own stages.

    WA_LIB=<libwhisper.so> python tools/load_probe.py [--repeat N] [--path device|host|both] [--chunk BYTES] MODEL ...

MODEL is a synthetic model of tools/wsynth.py ("small", "small:q5_1", "large-v3:q5_0", ...), written on first use; the file is read once
before the first load so that it sits in the page cache.  Every model is loaded N times per path.  The FIRST load of the process is printed
apart from the later ones: it pays the runtime's start-up (device initialisation, the code objects) whatever the loader does.  One JSON line
per model and path: wall times in ms, and - where the library has whisper_amd_load_stats - the stages of the median later load:
read = in loader->read, wait = waiting for the device, load = the whole wa_model_load, kernels = unpack kernels launched.
A library without the device path (no whisper_amd_load_stats) is timed on its only path whatever --path says."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wsynth, whisper_rs as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="+")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--path", choices=("device", "host", "both"), default="both")
    ap.add_argument("--chunk", type=int, default=None, help="WHISPER_AMD_LOAD_CHUNK for the device path")
    a = ap.parse_args()
    lib = W.load_library(os.environ.get("WA_LIB"))
    W.set_log_callback(lib, lambda l, t: None)
    has_stats = hasattr(lib, "whisper_amd_load_stats")
    paths = ["only"] if not has_stats else ["device", "host"] if a.path == "both" else [a.path]
    first = True
    for name in a.models:
        mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
        with open(mp, "rb") as f:           # page cache
            while f.read(1 << 26):
                pass
        for path in paths:
            os.environ.pop("WHISPER_AMD_LOAD_HOST", None); os.environ.pop("WHISPER_AMD_LOAD_CHUNK", None)
            if path == "host":
                os.environ["WHISPER_AMD_LOAD_HOST"] = "1"
            if path == "device" and a.chunk:
                os.environ["WHISPER_AMD_LOAD_CHUNK"] = str(a.chunk)
            walls, stats, first_ms = [], [], None
            for _ in range(a.repeat + (1 if first else 0)):
                t = time.perf_counter()
                ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(lib), lib=lib)
                ms = (time.perf_counter() - t) * 1e3
                s = ctx.load_stats() if has_stats else None
                ctx.free()
                if first:
                    first, first_ms = False, ms
                    continue
                walls.append(ms); stats.append(s)
            out = dict(model=name, file_mb=round(os.path.getsize(mp) / 1e6, 1), path=path, chunk=a.chunk if path == "device" else None,
                       first_load_of_process_ms=None if first_ms is None else round(first_ms, 1), later_ms=[round(w, 1) for w in walls])
            if walls:
                out["later_median_ms"] = round(statistics.median(walls), 1)
                out["later_spread_ms"] = round(max(walls) - min(walls), 1)
                if has_stats:
                    s = stats[walls.index(sorted(walls)[len(walls) // 2])]
                    assert s["path"] == (0 if path == "host" else 1), s
                    out.update(read_ms=round(s["read_us"] / 1e3, 1), wait_ms=round(s["wait_us"] / 1e3, 1), load_ms=round(s["load_us"] / 1e3, 1),
                               kernels=s["kernels"], tensor_mb=round(s["bytes_read"] / 1e6, 1))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
