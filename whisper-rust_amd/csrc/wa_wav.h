// wa_wav.h - the header of a RIFF/WAVE image in host memory: where the samples lie and what they are, in the terms the audio
// front end takes (wa_audio.h's format codes).  whisper_amd_wav_parse (wa_audio.cpp) is this function behind the C ABI.
//
// Plain C++ (no HIP, no allocation, no exception): tests/native/audio_formats_math.cpp compiles it with g++ alone.
//
// An image is "RIFF" size "WAVE" followed by chunks: a 4-byte id, a 4-byte little-endian size, the body, one pad byte where the size is odd.
// The walk stops at the first "data" chunk; a "fmt " chunk must come before it; every other chunk ("LIST", "fact", ...) is stepped over.
//   fmt  body: tag u16, channels u16, rate u32, bytes per second u32, nBlockAlign u16, bits u16, and for tag 0xFFFE (extensible) cbSize u16
//              (>= 22), valid bits u16, channel mask u32, a 16-byte sub-format GUID whose first two bytes are the real tag and whose last 14
//              bytes are 00 00 00 00 10 00 80 00 00 AA 00 38 9B 71; valid bits must equal the container's bits.
//   tag 1 with 8 / 16 / 24 / 32 bits -> U8 / I16 / S24 / S32; tag 3 with 32 / 64 -> F32 / F64; tag 6 with 8 -> ALAW; tag 7 with 8 -> ULAW.
//   nBlockAlign must be channels * bits / 8, and channels at least 1.  Channels and rate are reported as found: the entries refuse what they refuse.
//   data: the length is the smaller of the declared size and what the image holds behind the chunk header; a declared 0 or 0xFFFFFFFF (what a
//         writer that streams leaves) means "to the end of the image".  n_frames = that length / nBlockAlign, rounded down.
// Returns 0, or: -1 null or short arguments (no room for the 12-byte RIFF header); -2 not "RIFF" ... "WAVE" (RF64, RIFX); -3 a malformed chunk
// list - a chunk header or a body other than data's that runs past the image, a fmt body under 16 bytes, data before fmt; -4 an encoding that
// is none of the above; -5 no data chunk.  On failure *out is untouched.
#pragma once

#include "wa_audio.h"

#include <cstdint>
#include <cstring>

struct wa_wav_info {
    int64_t data_offset, n_frames;
    int32_t channels, sample_rate, format, bits;
};

inline uint32_t wa_wav_u16(const unsigned char * p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }
inline uint32_t wa_wav_u32(const unsigned char * p) { return wa_wav_u16(p) | (wa_wav_u16(p + 2) << 16); }

// tag and bits -> format code; -1: unsupported
inline int wa_wav_format(uint32_t tag, uint32_t bits) {
    if (tag == 1) return bits == 8 ? WA_AUDIO_U8 : bits == 16 ? WA_AUDIO_I16 : bits == 24 ? WA_AUDIO_S24 : bits == 32 ? WA_AUDIO_S32 : -1;
    if (tag == 3) return bits == 32 ? WA_AUDIO_F32 : bits == 64 ? WA_AUDIO_F64 : -1;
    if (tag == 6) return bits == 8 ? WA_AUDIO_ALAW : -1;
    if (tag == 7) return bits == 8 ? WA_AUDIO_ULAW : -1;
    return -1;
}

inline int wa_wav_parse(const void * image, int64_t size, wa_wav_info * out) {
    static const unsigned char guid_tail[14] = { 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71 };
    if (!image || !out || size < 12) return -1;
    const unsigned char * b = (const unsigned char *) image;
    if (memcmp(b, "RIFF", 4) != 0 || memcmp(b + 8, "WAVE", 4) != 0) return -2;
    wa_wav_info w = { 0, 0, 0, 0, -1, 0 };
    uint32_t block = 0;
    bool have_fmt = false;
    int64_t at = 12;
    while (at < size) {
        if (size - at < 8) return -3;                               // a chunk header cut off
        const unsigned char * c = b + at;
        const int64_t len = (int64_t) wa_wav_u32(c + 4), body = at + 8;
        if (memcmp(c, "data", 4) == 0) {
            if (!have_fmt) return -3;
            int64_t n = size - body;
            if (len != 0 && len != 0xFFFFFFFFLL && len < n) n = len;
            w.data_offset = body;
            w.n_frames = n / (int64_t) block;
            *out = w;
            return 0;
        }
        if (len > size - body) return -3;                           // a body that runs past the image
        if (memcmp(c, "fmt ", 4) == 0) {
            if (len < 16) return -3;
            const unsigned char * f = b + body;
            uint32_t tag = wa_wav_u16(f);
            const uint32_t channels = wa_wav_u16(f + 2), bits = wa_wav_u16(f + 14);
            block = wa_wav_u16(f + 12);
            if (tag == 0xFFFE) {
                if (len < 40 || wa_wav_u16(f + 16) < 22 || wa_wav_u16(f + 18) != bits || memcmp(f + 26, guid_tail, 14) != 0) return -4;
                tag = wa_wav_u16(f + 24);
            }
            const int format = wa_wav_format(tag, bits);
            if (format < 0 || channels == 0 || block != channels * bits / 8) return -4;
            w.channels = (int32_t) channels; w.sample_rate = (int32_t) wa_wav_u32(f + 4); w.format = format; w.bits = (int32_t) bits;
            have_fmt = true;
        }
        at = body + len + (len & 1);                                // the pad byte; past the end where the last chunk lacks it: the loop ends
    }
    return -5;
}
