// lphy_final.h — per-frame finalisation as device functions: sync word,
// Hamming(8,4) decode, sx1272 CRC (LoRaDecoder.cpp:7-21, phy.cpp:245-261).
// A workgroup stages its 256 frames' rows through LDS (finalize_block), else
// a thread per frame (finalize_frame).  Used by k_post (lphy_post.h) and by
// k_finalize (lphy_hip.hip: lphy_hip_decode_batch).
#pragma once
#include "lphy_args.h"

namespace {

// ---------------------------------------------------------------------------
// Per-frame finalisation: sync word, decode, CRC
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint8_t hamming84_decode(uint8_t b) {
    // LoRaCodes.hpp:250-281 (decodeHamming84sx): syndrome bits are the
    // parities of b & 0x17, 0x2E, 0x4B, 0x8D (b0^b1^b2^b4, b1^b2^b3^b5,
    // b0^b1^b3^b6, b0^b2^b3^b7); syndromes 0xD / 0x7 / 0xB / 0xE flip data
    // bit 0 / 1 / 2 / 3, read from a nibble table (all 256 inputs checked
    // against the switch form on the host)
    const unsigned x = b;
    const unsigned syn = (__builtin_popcount(x & 0x17u) & 1u) | ((__builtin_popcount(x & 0x2Eu) & 1u) << 1) |
                         ((__builtin_popcount(x & 0x4Bu) & 1u) << 2) | ((__builtin_popcount(x & 0x8Du) & 1u) << 3);
    constexpr unsigned long long kFlip = (1ull << 52) | (2ull << 28) | (4ull << 44) | (8ull << 56);
    return (uint8_t)((x ^ (unsigned)(kFlip >> (4 * syn))) & 0xfu);
}

// LoRaCodes.hpp:69-105
// The reference shifts the register 8 times through poly 0x1021 with a
// zero input bit per byte; that equals the byte-wise CCITT step with a
// zero input byte below (all 65,536 registers checked on the host), and
// the whitening register's feedback is the parity of v & 0xB8.
__device__ __forceinline__ unsigned sx_shift8(unsigned c) {
    unsigned x = c >> 8;
    x ^= x >> 4;
    return ((c << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xffffu;
}
__device__ __forceinline__ unsigned sx_lfsr(unsigned v) {
    return ((__builtin_popcount(v & 0xB8u) & 1u) | (v << 1)) & 0xffu;
}
__device__ __forceinline__ uint16_t sx1272_checksum(const uint8_t* data, int len) {
    auto shift8 = [](unsigned c) -> unsigned { return sx_shift8(c); };
    auto lfsr = [](unsigned v) -> unsigned { return sx_lfsr(v); };
    unsigned res = 0, v = 0xff;
    for (int i = 0; i < len; ++i) {
        const unsigned crc = shift8(res);
        v = lfsr(v);
        res = crc ^ data[i];
    }
    res ^= v;
    v = lfsr(v);
    res ^= v << 8;
    return (uint16_t)res;
}



// Register form of the finalisation for rows of up to 64 symbols (32
// bytes) that are 16-byte aligned with 4-aligned output: the record and all
// the symbols are loaded before the status test (one memory round trip, not
// two), and the checksum runs over the decoded words held in registers
// instead of re-reading the bytes just stored (a third round trip and 28
// byte loads per frame).  Same bytes, same checksum steps as below.
__device__ __forceinline__ bool finalize_frame_regs(const FinalArgs& A, unsigned long long f) {
    const unsigned long long nb = A.nsyms / 2;
    const uint16_t* s = A.syms + f * A.sym_stride;
    uint8_t* out = A.bytes + f * nb;
    if (!A.decode || (A.nsyms & 1) || nb > 32 || (nb & 3) || (reinterpret_cast<uintptr_t>(s) & 15) ||
        (reinterpret_cast<uintptr_t>(out) & 3))
        return false;
    const unsigned nw = (unsigned)(nb / 4);  // wave-uniform
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4 q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if ((unsigned)j < nw) q[j] = s4[j];
    lphy_frame_meta m = A.meta[f];
    if (m.status != 0) return true;
    if (A.set_sync && m.have_sync)
        m.sync_word = (uint8_t)((((m.sw0 >> A.shift) & 0x0f) << 4) | ((m.sw1 >> A.shift) & 0x0f));
    unsigned wd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        wd[j] = 0u;
        if ((unsigned)j < nw) {
            const unsigned qs[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned hi = hamming84_decode((uint8_t)qs[b]) & 0x0fu;
                const unsigned lo = hamming84_decode((uint8_t)(qs[b] >> 16)) & 0x0fu;
                wd[j] |= ((hi << 4) | lo) << (8 * b);
            }
            *reinterpret_cast<unsigned*>(out + 4 * j) = wd[j];
        }
    }
    if (nb >= 4) {  // phy.cpp:252-259, over bytes 2 .. nb-3
        const int len = (int)nb - 4;
        unsigned res = 0, v = 0xff;
#pragma unroll
        for (int i = 0; i < 28; ++i) {
            if (i >= len) break;  // wave-uniform
            const unsigned byte = (wd[(i + 2) >> 2] >> (8 * ((i + 2) & 3))) & 0xffu;
            const unsigned crc = sx_shift8(res);
            v = sx_lfsr(v);
            res = crc ^ byte;
        }
        res ^= v;
        v = sx_lfsr(v);
        res ^= v << 8;
        const unsigned pw = wd[(nb - 2) >> 2] >> (8 * ((nb - 2) & 3));  // bytes nb-2, nb-1 (same word)
        m.crc_ok = (uint16_t)(pw & 0xffffu) == (uint16_t)res;
    } else {
        m.crc_ok = 0;
    }
    A.meta[f] = m;
    return true;
}

__device__ __forceinline__ void finalize_frame(const FinalArgs& A, unsigned long long f) {
    if (finalize_frame_regs(A, f)) return;
    lphy_frame_meta m = A.meta[f];
    if (m.status != 0) return;
    if (A.set_sync && m.have_sync)
        m.sync_word = (uint8_t)((((m.sw0 >> A.shift) & 0x0f) << 4) | ((m.sw1 >> A.shift) & 0x0f));
    if (A.decode) {
        if (A.nsyms & 1) {
            m.status = -EINVAL;  // LoRaDecoder.cpp:10
        } else {
            const unsigned long long nb = A.nsyms / 2;
            const uint16_t* s = A.syms + f * A.sym_stride;
            uint8_t* out = A.bytes + f * nb;
            unsigned long long k0 = 0;
            // 8 symbols per 16-byte load and 4 bytes per store where aligned
            // (the bench rows: 64 symbols in, 32 bytes out)
            if ((reinterpret_cast<uintptr_t>(s) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
                const uint4* s4 = reinterpret_cast<const uint4*>(s);
                for (; k0 + 4 <= nb; k0 += 4) {
                    const uint4 q = s4[k0 / 4];
                    const unsigned qs[4] = {q.x, q.y, q.z, q.w};
                    unsigned wd = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned hi = hamming84_decode((uint8_t)qs[j]) & 0x0fu;
                        const unsigned lo = hamming84_decode((uint8_t)(qs[j] >> 16)) & 0x0fu;
                        wd |= ((hi << 4) | lo) << (8 * j);
                    }
                    *reinterpret_cast<unsigned*>(out + k0) = wd;
                }
            }
            for (unsigned long long k = k0; k < nb; ++k) {
                const uint8_t hi = hamming84_decode((uint8_t)s[2 * k]) & 0x0f;
                const uint8_t lo = hamming84_decode((uint8_t)s[2 * k + 1]) & 0x0f;
                out[k] = (uint8_t)((hi << 4) | lo);
            }
            if (nb >= 4) {  // phy.cpp:252-259
                const uint16_t provided = (uint16_t)(out[nb - 2] | (out[nb - 1] << 8));
                m.crc_ok = provided == sx1272_checksum(out + 2, (int)(nb - 4));
            } else {
                m.crc_ok = 0;
            }
        }
    }
    A.meta[f] = m;
}

// A workgroup's 256 rows at once (the register form's rows: 8 to 64
// symbols, a multiple of 8, 16-byte aligned): the symbols come in and the
// bytes go out as whole contiguous rows across the workgroup, staged in LDS,
// instead of each thread's 128-byte row at a 128-byte lane stride; each
// thread then decodes its frame as finalize_frame_regs does (same bytes,
// same checksum steps).  Rows of a non-zero status are left as they are.
struct FinStage {
    uint4 in[kTile * 9];      // 9 x 16 B per row (8 used): conflict-free 16-byte reads
    unsigned out[kTile * 9];  // the decoded words
    unsigned char ok[kTile];  // the row was decoded
};
__device__ __forceinline__ bool finalize_block(const FinalArgs& A, unsigned long long f0, FinStage& st) {
    const unsigned long long nb = A.nsyms / 2;
    if (!A.decode || (A.nsyms & 1) || nb < 4 || nb > 32 || (nb & 3) || (A.sym_stride & 7) ||
        (reinterpret_cast<uintptr_t>(A.syms) & 15) || (reinterpret_cast<uintptr_t>(A.bytes) & 3) ||
        f0 >= A.frames)
        return false;  // (uniform over the workgroup)
    const unsigned nw = (unsigned)(nb / 4);
    const unsigned nf = A.frames - f0 < (unsigned long long)kTile ? (unsigned)(A.frames - f0) : (unsigned)kTile;
    const unsigned t = threadIdx.x;
    for (unsigned i = t; i < nf * nw; i += kTile) {
        const unsigned fr = i / nw, k = i - fr * nw;
        st.in[fr * 9 + k] = reinterpret_cast<const uint4*>(A.syms + (f0 + fr) * A.sym_stride)[k];
    }
    __syncthreads();
    if (t < nf) {
        const unsigned long long f = f0 + t;
        lphy_frame_meta m = A.meta[f];
        const bool ok = m.status == 0;
        st.ok[t] = ok ? 1 : 0;
        if (ok) {
            if (A.set_sync && m.have_sync)
                m.sync_word = (uint8_t)((((m.sw0 >> A.shift) & 0x0f) << 4) | ((m.sw1 >> A.shift) & 0x0f));
            unsigned wd[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                wd[j] = 0u;
                if ((unsigned)j < nw) {
                    const uint4 q = st.in[t * 9 + j];
                    const unsigned qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const unsigned hi = hamming84_decode((uint8_t)qs[b]) & 0x0fu;
                        const unsigned lo = hamming84_decode((uint8_t)(qs[b] >> 16)) & 0x0fu;
                        wd[j] |= ((hi << 4) | lo) << (8 * b);
                    }
                    st.out[t * 9 + j] = wd[j];
                }
            }
            // phy.cpp:252-259, over bytes 2 .. nb-3 (finalize_frame_regs)
            const int len = (int)nb - 4;
            unsigned res = 0, v = 0xff;
#pragma unroll
            for (int i = 0; i < 28; ++i) {
                if (i >= len) break;  // uniform
                const unsigned byte = (wd[(i + 2) >> 2] >> (8 * ((i + 2) & 3))) & 0xffu;
                const unsigned crc = sx_shift8(res);
                v = sx_lfsr(v);
                res = crc ^ byte;
            }
            res ^= v;
            v = sx_lfsr(v);
            res ^= v << 8;
            const unsigned pw = st.out[t * 9 + (unsigned)((nb - 2) >> 2)] >> (8 * ((nb - 2) & 3));
            m.crc_ok = (uint16_t)(pw & 0xffffu) == (uint16_t)res;
            A.meta[f] = m;
        }
    }
    __syncthreads();
    for (unsigned i = t; i < nf * nw; i += kTile) {
        const unsigned fr = i / nw, k = i - fr * nw;
        if (st.ok[fr]) reinterpret_cast<unsigned*>(A.bytes + (f0 + fr) * nb)[k] = st.out[fr * 9 + k];
    }
    return true;
}

}  // namespace
