// wa_quantw.cpp - the public entries of weight quantisation (include/whisper_amd.h):
//   whisper_amd_quantize_rows: F32 / F16 values -> ggml weight blocks through the kernels of wa_quantw.hip (where = 1) or the host statement
//     wa_quantw.h (where = 0);
//   whisper_amd_quantize_file / _loader and whisper_amd_init_from_file_quantized / whisper_amd_init_quantized_with_params: both read an F16 / F32
//     model through ONE transcoder (qw_transcoder below), a whisper_model_loader that yields, piece by piece, the bytes of the file the reference's
//     quantize tool would write.  The file writer drains it into a file; quantise-at-load hands it to the unchanged wa_model_load, so the context is
//     the one loaded from that file by construction.  Tensor bytes go in chunks of 1 Mi values: pinned buffer -> device -> wa_launch_quantw -> pinned
//     buffer; with WHISPER_AMD_LOAD_HOST=1 (or without pinned / device buffers) the host statement quantises instead.  Both give the same bytes.
#include "wa_internal.h"
#include "wa_quantw.h"
#include "wa_quantw_launch.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace {

bool on_device(const void * p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void) hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice;
}

const char * type_name(int type) {
    switch (type) {
        case 2: return "Q4_0"; case 3: return "Q4_1"; case 6: return "Q5_0"; case 7: return "Q5_1"; case 8: return "Q8_0";
        case 10: return "Q2_K"; case 11: return "Q3_K"; case 12: return "Q4_K"; case 13: return "Q5_K"; case 14: return "Q6_K";
    }
    return "?";
}

// a type this library quantises; logs why not
bool type_ok(const char * who, int type) {
    if (type == 10 || type == 11) {
        WA_ERROR("%s: %s is not quantised here (its searches - make_q3_quants, make_qp_quants, the MAD walk - are out of scope)\n", who, type_name(type));
        return false;
    }
    if (!wa_qw_block_values(type)) { WA_ERROR("%s: ggml type %d is not a weight format this library quantises\n", who, type); return false; }
    return true;
}

// the reference tool's ftype number (ggml_ftype) of a weight type
int ftype_of(int type) { return type == 6 ? 8 : type == 7 ? 9 : type == 8 ? 7 : type; }

constexpr size_t QW_CHUNK_VALUES = (size_t) 1 << 20;      // values per quantise launch (a multiple of 256), and bytes / 4 of a copied-through piece

// The device side of a run of launches: one stream, a pinned and a device buffer each way, the flag word.  Freed on every way out.
struct qw_device {
    hipStream_t stream = nullptr;
    uint8_t * pin_in = nullptr, * pin_out = nullptr, * d_out = nullptr;
    void * d_in = nullptr;
    uint32_t * d_flag = nullptr;
    static constexpr size_t IN = QW_CHUNK_VALUES * 4, OUT = QW_CHUNK_VALUES / 32 * 34;

    bool open() {
        const uint32_t zero = 0;
        const bool got = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess && hipHostMalloc((void **) &pin_in, IN, hipHostMallocDefault) == hipSuccess &&
                         hipHostMalloc((void **) &pin_out, OUT + 16, hipHostMallocDefault) == hipSuccess && hipMalloc(&d_in, IN) == hipSuccess &&
                         hipMalloc((void **) &d_out, OUT) == hipSuccess && hipMalloc((void **) &d_flag, 4) == hipSuccess &&
                         hipMemcpy(d_flag, &zero, 4, hipMemcpyHostToDevice) == hipSuccess;
        if (!got) { (void) hipGetLastError(); close(); }
        return got;
    }
    // n values in pin_in -> blocks in pin_out.  0, 3: a value that is not finite, -1: a HIP call failed (logged)
    int run(int type, bool f16, size_t n) {
        const size_t nblk = n / (size_t) wa_qw_block_values(type), out_bytes = nblk * wa_qw_block_bytes(type);
        uint32_t * flag = (uint32_t *) (pin_out + OUT);
        if (!WA_HIP_OK(hipMemcpyAsync(d_in, pin_in, n * (f16 ? 2 : 4), hipMemcpyHostToDevice, stream)) ||
            !WA_HIP_OK((hipError_t) wa_launch_quantw(stream, type, d_in, f16 ? 1 : 0, nblk, d_out, d_flag)) ||
            !WA_HIP_OK(hipMemcpyAsync(pin_out, d_out, out_bytes, hipMemcpyDeviceToHost, stream)) ||
            !WA_HIP_OK(hipMemcpyAsync(flag, d_flag, 4, hipMemcpyDeviceToHost, stream)) || !WA_HIP_OK(hipStreamSynchronize(stream))) return -1;
        return *flag ? 3 : 0;      // the flag is only ever set: the first refusal ends the run
    }
    void close() {
        if (stream) (void) hipStreamSynchronize(stream);
        if (pin_in) (void) hipHostFree(pin_in);
        if (pin_out) (void) hipHostFree(pin_out);
        if (d_in) (void) hipFree(d_in);
        if (d_out) (void) hipFree(d_out);
        if (d_flag) (void) hipFree(d_flag);
        if (stream) (void) hipStreamDestroy(stream);
        pin_in = pin_out = d_out = nullptr; d_in = nullptr; d_flag = nullptr; stream = nullptr;
    }
    ~qw_device() { close(); }
};

// An F16 / F32 model read from `in`, presented as the quantised file (what examples/quantize writes): the header with ftype = 2 * 1000 + ftype,
// mel filters and vocabulary unchanged, every tensor record in order - quantised where it is 2-D, F16 or F32 and none of the four names the
// tool skips (the two positional embeddings, the two conv biases, which the converters write as [d, 1]), all of it as one row of nelements values.
struct qw_transcoder {
    whisper_model_loader * in;
    int type;
    bool host = false, failed = false, done = false, header_sent = false;
    std::vector<uint8_t> out, tmp;
    size_t pos = 0;
    int64_t left = 0, n_kernels = 0;      // of the current tensor: values (quantised) or bytes (copied) still to come
    bool quant = false, f16 = false;
    std::string name;
    qw_device dev;

    qw_transcoder(whisper_model_loader * in_, int type_, int device) : in(in_), type(type_) {
        const char * e = getenv("WHISPER_AMD_LOAD_HOST");
        host = e && *e && strcmp(e, "0") != 0;
        if (!host && (hipSetDevice(device) != hipSuccess || !dev.open())) {
            (void) hipGetLastError();
            WA_WARN("%s: no pinned / device buffers - quantising on the host\n", __func__);
            host = true;
        }
    }
    bool get(void * p, size_t n) { return in->read(in->context, p, n) == n; }
    void put(const void * p, size_t n) { out.insert(out.end(), (const uint8_t *) p, (const uint8_t *) p + n); }
    bool fail(const char * what) { WA_ERROR("quantize: %s\n", what); failed = true; return false; }

    bool header() {
        uint32_t magic = 0;
        int32_t hp[11];
        if (!get(&magic, 4) || magic != 0x67676d6c) return fail("invalid model data (bad magic)");
        if (!get(hp, sizeof(hp))) return fail("truncated header");
        if (hp[10] % 1000 != 1 && hp[10] % 1000 != 0) {
            WA_ERROR("quantize: the model is already quantised (ftype %d); an F16 or F32 model is needed\n", hp[10]);
            failed = true; return false;
        }
        hp[10] = 2 * 1000 + ftype_of(type);      // GGML_QNT_VERSION * GGML_QNT_VERSION_FACTOR + ftype
        put(&magic, 4); put(hp, sizeof(hp));
        int32_t n_mel = 0, n_fft = 0, n_vocab = 0;
        if (!get(&n_mel, 4) || !get(&n_fft, 4) || n_mel <= 0 || n_fft <= 0 || n_mel > 1024 || n_fft > 4096) return fail("invalid mel filter header");
        put(&n_mel, 4); put(&n_fft, 4);
        tmp.resize((size_t) n_mel * n_fft * 4);
        if (!get(tmp.data(), tmp.size())) return fail("truncated mel filters");
        put(tmp.data(), tmp.size());
        if (!get(&n_vocab, 4) || n_vocab < 0 || n_vocab > (1 << 24)) return fail("invalid vocab size");
        put(&n_vocab, 4);
        for (int i = 0; i < n_vocab; ++i) {
            uint32_t len = 0;
            if (!get(&len, 4) || len > (1u << 20)) return fail("invalid vocab entry");
            put(&len, 4);
            tmp.resize(len);
            if (len && !get(tmp.data(), len)) return fail("truncated vocab");
            put(tmp.data(), len);
        }
        header_sent = true;
        return true;
    }
    bool record() {
        int32_t n_dims = 0, length = 0, ttype = 0, ne[4] = { 1, 1, 1, 1 };
        if (!get(&n_dims, 4)) { if (in->eof(in->context)) { done = true; return false; } return fail("truncated tensor header"); }
        if (!get(&length, 4) || !get(&ttype, 4) || n_dims < 1 || n_dims > 4 || length <= 0 || length > 256) return fail("corrupt tensor header");
        int64_t nel = 1;
        for (int i = 0; i < n_dims; ++i) {
            if (!get(&ne[i], 4) || ne[i] <= 0 || (nel *= ne[i]) > ((int64_t) 1 << 40)) return fail("corrupt tensor shape");
        }
        name.assign((size_t) length, '\0');
        if (!get(&name[0], (size_t) length)) return fail("truncated tensor name");
        if (ttype != 0 && ttype != 1) { WA_ERROR("quantize: tensor '%s' has type %d; only F32 and F16 tensors can be read\n", name.c_str(), ttype); failed = true; return false; }
        quant = n_dims == 2 && name != "encoder.positional_embedding" && name != "decoder.positional_embedding" && name != "encoder.conv1.bias" && name != "encoder.conv2.bias";
        f16 = ttype == 1;
        const int bv = wa_qw_block_values(type);
        if (quant && ne[0] % bv != 0) {
            WA_ERROR("quantize: tensor '%s' has rows of %d values, no multiple of %s's block of %d\n", name.c_str(), ne[0], type_name(type), bv);
            failed = true; return false;
        }
        const int32_t ttype_out = quant ? type : ttype;
        put(&n_dims, 4); put(&length, 4); put(&ttype_out, 4);
        for (int i = 0; i < n_dims; ++i) put(&ne[i], 4);
        put(name.data(), name.size());
        left = quant ? nel : nel * (f16 ? 2 : 4);
        return true;
    }
    bool data() {
        if (!quant) {
            const size_t k = (size_t) std::min<int64_t>(left, (int64_t) QW_CHUNK_VALUES * 4);
            out.resize(k);
            if (!get(out.data(), k)) { out.clear(); WA_ERROR("quantize: truncated tensor '%s'\n", name.c_str()); failed = true; return false; }
            left -= (int64_t) k;
            return true;
        }
        const size_t n = (size_t) std::min<int64_t>(left, (int64_t) QW_CHUNK_VALUES), in_bytes = n * (f16 ? 2 : 4);
        const size_t out_bytes = n / (size_t) wa_qw_block_values(type) * wa_qw_block_bytes(type);
        if (host) tmp.resize(in_bytes);
        uint8_t * src = host ? tmp.data() : dev.pin_in;
        if (!get(src, in_bytes)) { WA_ERROR("quantize: truncated tensor '%s'\n", name.c_str()); failed = true; return false; }
        out.resize(out_bytes);
        int rc;
        if (host) rc = f16 ? wa_quantw_rows_f16(type, (const uint16_t *) src, (int64_t) n, out.data()) : wa_quantw_rows(type, (const float *) src, (int64_t) n, out.data());
        else { rc = dev.run(type, f16, n); n_kernels++; if (rc == 0) memcpy(out.data(), dev.pin_out, out_bytes); }
        if (rc != 0) {
            out.clear();
            if (rc == 3) WA_ERROR("quantize: tensor '%s' holds a value that is not finite\n", name.c_str());
            failed = true; return false;
        }
        left -= (int64_t) n;
        return true;
    }
    size_t read(void * dst, size_t n) {
        size_t got = 0;
        while (got < n) {
            if (pos == out.size()) {
                if (failed || done) break;
                out.clear(); pos = 0;
                if (!(!header_sent ? header() : left == 0 ? record() : data())) break;
                continue;
            }
            const size_t k = std::min(n - got, out.size() - pos);
            memcpy((uint8_t *) dst + got, out.data() + pos, k);
            got += k; pos += k;
        }
        return got;
    }
    whisper_model_loader loader() {
        whisper_model_loader l;
        l.context = this;
        l.read  = [](void * c, void * o, size_t n) { return ((qw_transcoder *) c)->read(o, n); };
        l.eof   = [](void * c) { auto * t = (qw_transcoder *) c; return t->pos == t->out.size() && (t->done || t->failed); };
        l.close = [](void * c) { auto * t = (qw_transcoder *) c; if (t->in) { t->in->close(t->in->context); t->in = nullptr; } };
        return l;
    }
};

struct qw_file { FILE * f; bool eof; };
whisper_model_loader file_loader(qw_file * src) {
    whisper_model_loader l;
    l.context = src;
    l.read  = [](void * c, void * out, size_t n) { auto * s = (qw_file *) c; size_t r = fread(out, 1, n, s->f); if (r < n) s->eof = true; return r; };
    l.eof   = [](void * c) { return ((qw_file *) c)->eof; };
    l.close = [](void * c) { auto * s = (qw_file *) c; if (s->f) { fclose(s->f); s->f = nullptr; } };
    return l;
}

} // namespace

extern "C" {

int whisper_amd_quantize_rows(int type, const void * src, int src_is_f16, int64_t n, void * dst, int where) {
    if (!type_ok(__func__, type)) return WHISPER_AMD_QUANTIZE_REFUSED;
    const int bv = wa_qw_block_values(type);
    if (!src || !dst || n < 0 || (where != 0 && where != 1)) { WA_ERROR("%s: refused (type %d, n %lld, where %d)\n", __func__, type, (long long) n, where); return WHISPER_AMD_QUANTIZE_REFUSED; }
    if (n % bv != 0) { WA_ERROR("%s: %lld values are no multiple of %s's block of %d\n", __func__, (long long) n, type_name(type), bv); return WHISPER_AMD_QUANTIZE_REFUSED; }
    if (n == 0) return 0;
    if (where == 0) {      // the host statement: nothing of HIP is touched
        const int rc = src_is_f16 ? wa_quantw_rows_f16(type, (const uint16_t *) src, n, dst) : wa_quantw_rows(type, (const float *) src, n, dst);
        if (rc == 3) { WA_ERROR("%s: a value that is not finite\n", __func__); return WHISPER_AMD_QUANTIZE_NOT_FINITE; }
        return rc ? WHISPER_AMD_QUANTIZE_REFUSED : 0;
    }
    const size_t nblk = (size_t) (n / bv), out_bytes = nblk * wa_qw_block_bytes(type), in_bytes = (size_t) n * (src_is_f16 ? 2 : 4);
    struct bufs {      // what this one call needs on the device, freed on every way out
        void * src = nullptr; uint8_t * dst = nullptr; uint32_t * flag = nullptr; hipStream_t stream = nullptr;
        ~bufs() { if (src) (void) hipFree(src); if (dst) (void) hipFree(dst); if (flag) (void) hipFree(flag); if (stream) (void) hipStreamDestroy(stream); }
    } b;
    const bool src_dev = on_device(src);      // managed memory counts as host memory: it gets the staged copy
    if (!WA_HIP_OK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking))) return WHISPER_AMD_QUANTIZE_FAILED;
    const void * dsrc = src;
    if (!src_dev || ((uintptr_t) src & 15) != 0) {      // host values, or device values the 16-byte loads cannot take where they lie: a staged copy
        if (!WA_HIP_OK(hipMalloc(&b.src, in_bytes)) ||
            !WA_HIP_OK(hipMemcpyAsync(b.src, src, in_bytes, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b.stream))) return WHISPER_AMD_QUANTIZE_FAILED;
        dsrc = b.src;
    }
    uint32_t flag = 0;
    if (!WA_HIP_OK(hipMalloc((void **) &b.dst, out_bytes)) || !WA_HIP_OK(hipMalloc((void **) &b.flag, 4)) ||
        !WA_HIP_OK(hipMemcpyAsync(b.flag, &flag, 4, hipMemcpyHostToDevice, b.stream)) ||
        !WA_HIP_OK((hipError_t) wa_launch_quantw(b.stream, type, dsrc, src_is_f16, nblk, b.dst, b.flag)) ||
        !WA_HIP_OK(hipMemcpyAsync(&flag, b.flag, 4, hipMemcpyDeviceToHost, b.stream)) ||
        !WA_HIP_OK(hipMemcpyAsync(dst, b.dst, out_bytes, hipMemcpyDeviceToHost, b.stream)) ||
        !WA_HIP_OK(hipStreamSynchronize(b.stream))) return WHISPER_AMD_QUANTIZE_FAILED;
    if (flag) { WA_ERROR("%s: a value that is not finite\n", __func__); return WHISPER_AMD_QUANTIZE_NOT_FINITE; }
    return 0;
}

int whisper_amd_quantize_loader(struct whisper_model_loader * loader, const char * path_out, int type) {
    if (!loader) return WHISPER_AMD_QUANTIZE_REFUSED;
    if (!type_ok(__func__, type) || !path_out) { loader->close(loader->context); return WHISPER_AMD_QUANTIZE_REFUSED; }
    int rc = WHISPER_AMD_QUANTIZE_FAILED;
    try {
        qw_transcoder t(loader, type, 0);
        whisper_model_loader l = t.loader();
        FILE * f = fopen(path_out, "wb");
        if (!f) WA_ERROR("%s: failed to open '%s' for writing\n", __func__, path_out);
        std::vector<uint8_t> buf((size_t) 1 << 20);
        bool wrote = f != nullptr;
        while (wrote) {
            const size_t k = t.read(buf.data(), buf.size());
            if (k && fwrite(buf.data(), 1, k, f) != k) { WA_ERROR("%s: write to '%s' failed\n", __func__, path_out); wrote = false; }
            if (k < buf.size()) break;
        }
        if (f && fclose(f) != 0) wrote = false;
        l.close(l.context);
        rc = wrote && t.done && !t.failed ? 0 : t.failed ? WHISPER_AMD_QUANTIZE_REFUSED : WHISPER_AMD_QUANTIZE_FAILED;
        if (rc != 0 && f) remove(path_out);
    } catch (const std::exception & e) {
        WA_ERROR("%s: %s\n", __func__, e.what());
    }
    return rc;
}

int whisper_amd_quantize_file(const char * path_in, const char * path_out, int type) {
    qw_file src{ path_in ? fopen(path_in, "rb") : nullptr, false };
    if (!src.f) { WA_ERROR("%s: failed to open '%s'\n", __func__, path_in ? path_in : "(null)"); return WHISPER_AMD_QUANTIZE_REFUSED; }
    setvbuf(src.f, nullptr, _IOFBF, 1 << 22);
    whisper_model_loader l = file_loader(&src);
    return whisper_amd_quantize_loader(&l, path_out, type);
}

struct whisper_context * whisper_amd_init_quantized_with_params(struct whisper_model_loader * loader, struct whisper_context_params cparams, int type) {
    if (!loader) return nullptr;
    if (!type_ok(__func__, type)) { loader->close(loader->context); return nullptr; }
    whisper_context * ctx = nullptr;
    try {
        qw_transcoder t(loader, type, cparams.gpu_device);
        whisper_model_loader l = t.loader();
        ctx = whisper_init_with_params(&l, cparams);      // closes l, and with it the caller's loader
        l.close(l.context);
        if (ctx) ctx->load_stats[2] += t.n_kernels;      // the quantise launches count among the unpack kernels
    } catch (const std::exception & e) {
        WA_ERROR("%s: %s\n", __func__, e.what());
    }
    return ctx;
}

struct whisper_context * whisper_amd_init_from_file_quantized(const char * path, struct whisper_context_params cparams, int type) {
    WA_INFO("%s: loading model from '%s' as %s\n", __func__, path ? path : "(null)", type_name(type));
    qw_file src{ path ? fopen(path, "rb") : nullptr, false };
    if (!src.f) { WA_ERROR("%s: failed to open '%s'\n", __func__, path ? path : "(null)"); return nullptr; }
    setvbuf(src.f, nullptr, _IOFBF, 1 << 22);
    whisper_model_loader l = file_loader(&src);
    whisper_context * ctx = whisper_amd_init_quantized_with_params(&l, cparams, type);
    if (ctx) ctx->path_model = path;
    return ctx;
}

} // extern "C"
