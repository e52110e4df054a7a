// lphy_lorawan.hip — the LoRaWAN MAC helpers of the reference
// (src/lorawan/lorawan.cpp) batched on the GPU:
// compute_mic (lorawan.cpp:35-98: AES-128 CMAC over B0 || data) for many
// frames, and parse_frame's checks (lorawan.cpp:150-176) on the decoded
// bytes the demodulator leaves in HBM.  Bit-exact to the reference
// (tests/test_gpu_lorawan.py against the oracle, which
// tests/test_oracle_vs_reference.py pins to lorawan.cpp + tiny-AES).
//
// One thread per frame: a CMAC is a chain of AES blocks, so the parallelism
// is across frames.  AES-128 runs from one 1 KiB "T-table" (SubBytes and
// MixColumns of one input byte, LoRa-independent FIPS-197 algebra) held in
// LDS as 32 replicas, entry x of replica c at dword 32x + c: lane l reads
// replica l & 31, so the 32 lanes of a ds_read_b32 group always hit 32
// different banks whatever bytes they look up (no conflicts).  The other
// three tables are byte rotations of the first (v_alignbit).  The table is
// derived in the prologue from the field inverse, not loaded.  Round keys
// (44 dwords) live in VGPRs.  Each workgroup loops over frames
// (grid-stride), so the 32 KiB table build is paid once per workgroup.
//
// The same two jobs on the lphy_ragged_desc table of the ragged PHY calls:
// build_frame (lorawan.cpp:100-136) for frames of different lengths packed at
// byte granularity (k_lw_build: header, FOpts and FRMPayload gathered, MIC
// appended, lora_encode's symbols on request), and parse_frame's checks on
// what lphy_hip_demod_ragged left, with the key found by DevAddr in a sorted
// session table (k_lw_parse_ragged).  The TU knows no context: the samples of
// a symbol are an argument.
//
// And the FRMPayload cipher of LoRaWAN 1.0.x 4.3.3, which the reference does
// not have (k_lw_crypt): a keystream of independent AES blocks XORed over byte
// ranges in place, in front of k_lw_build and behind k_lw_parse_ragged on the
// same table, or on plain descriptors.  Here the parallelism is across 16-byte
// blocks as well as across ranges: a group of lanes shares a range.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>

#include "../../include/lphy_hip.h"
#include "lphy_lorawan_ragged.h"

namespace {

using namespace lphy;

#define LW_OK(x)                                                           \
    do {                                                                   \
        hipError_t e_ = (x);                                               \
        if (e_ != hipSuccess) {                                            \
            fprintf(stderr, "lphy_lorawan: %s failed: %s (%s:%d)\n", #x,   \
                    hipGetErrorString(e_), __FILE__, __LINE__);            \
            return -EIO;                                                   \
        }                                                                  \
    } while (0)

constexpr unsigned kThreads = 256;
constexpr unsigned kCopies = 32;
constexpr unsigned kMaxBlocks = 2048;  // 8 workgroups per CU, grid-stride beyond

// ---------------------------------------------------------------- AES-128
__device__ __forceinline__ unsigned gmul2(unsigned a) { return ((a << 1) ^ ((a & 0x80) ? 0x1B : 0)) & 0xFF; }

__device__ unsigned gmul(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int i = 0; i < 8; ++i) {
        if (b & 1) r ^= a;
        a = gmul2(a);
        b >>= 1;
    }
    return r;
}

// S-box entry by definition: affine map of the inverse in GF(2^8).
__device__ unsigned sbox_entry(unsigned x) {
    unsigned inv = 1, p = x;
    for (int e = 254; e; e >>= 1) {
        if (e & 1) inv = gmul(inv, p);
        p = gmul(p, p);
    }
    if (!x) inv = 0;
    unsigned y = 0x63;
    for (int k = 0; k < 5; ++k) y ^= ((inv << k) | (inv >> ((8 - k) & 7))) & 0xFF;
    return y;
}

// T[x] for byte row 0 of a column, little-endian packed: (2s, s, s, 3s).
__device__ void build_table(uint32_t* lds) {
    for (unsigned x = threadIdx.x; x < 256; x += blockDim.x) {
        const unsigned s = sbox_entry(x), s2 = gmul2(s);
        const uint32_t t = s2 | (s << 8) | (s << 16) | ((s2 ^ s) << 24);
        for (unsigned c = 0; c < kCopies; ++c) lds[x * kCopies + c] = t;
    }
    __syncthreads();
}

struct Tab {
    const uint32_t* t;  // this lane's replica
    __device__ __forceinline__ uint32_t T(uint32_t x) const { return t[x * kCopies]; }
    __device__ __forceinline__ uint32_t S(uint32_t x) const { return (t[x * kCopies] >> 8) & 0xFF; }
};

__device__ __forceinline__ uint32_t rotl(uint32_t v, unsigned r) { return __builtin_amdgcn_alignbit(v, v, 32 - r); }
__device__ __forceinline__ uint32_t byte_of(uint32_t v, unsigned k) { return (v >> (8 * k)) & 0xFF; }

// FIPS-197 5.2 key expansion; words little-endian (key byte 4i in bits 0-7).
__device__ __forceinline__ void expand_key(const Tab& tb, const uint32_t k[4], uint32_t rk[44]) {
    constexpr uint32_t rcon[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
#pragma unroll
    for (int i = 0; i < 4; ++i) rk[i] = k[i];
#pragma unroll
    for (int i = 4; i < 44; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 4 == 0)  // SubWord(RotWord(t)) ^ Rcon
            t = (tb.S(byte_of(t, 1)) | tb.S(byte_of(t, 2)) << 8 | tb.S(byte_of(t, 3)) << 16 |
                 tb.S(byte_of(t, 0)) << 24) ^ rcon[i / 4 - 1];
        rk[i] = rk[i - 4] ^ t;
    }
}

// FIPS-197 5.1 cipher: new column c takes row r from old column c + r
// (ShiftRows); rows 1-3 of the MixColumns contribution are the row-0 table
// rotated by 8r bits.
__device__ __forceinline__ void encrypt(const Tab& tb, const uint32_t rk[44], uint32_t s[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] ^= rk[c];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        uint32_t t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            t[c] = tb.T(byte_of(s[c], 0)) ^ rotl(tb.T(byte_of(s[(c + 1) & 3], 1)), 8) ^
                   rotl(tb.T(byte_of(s[(c + 2) & 3], 2)), 16) ^ rotl(tb.T(byte_of(s[(c + 3) & 3], 3)), 24) ^
                   rk[4 * r + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = t[c];
    }
    uint32_t t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        t[c] = (tb.S(byte_of(s[c], 0)) | tb.S(byte_of(s[(c + 1) & 3], 1)) << 8 |
                tb.S(byte_of(s[(c + 2) & 3], 2)) << 16 | tb.S(byte_of(s[(c + 3) & 3], 3)) << 24) ^
               rk[40 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = t[c];
}

// CMAC doubling of a little-endian-packed block read as one big-endian
// 128-bit number (lorawan.cpp:15-31).
__device__ __forceinline__ void cmac_double(const uint32_t in[4], uint32_t out[4]) {
    uint32_t b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = __builtin_bswap32(in[i]);
    const uint32_t msb = b[0] >> 31;
    uint32_t o[4];
    o[0] = (b[0] << 1) | (b[1] >> 31);
    o[1] = (b[1] << 1) | (b[2] >> 31);
    o[2] = (b[2] << 1) | (b[3] >> 31);
    o[3] = (b[3] << 1) ^ (msb ? 0x87u : 0u);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = __builtin_bswap32(o[i]);
}

// Up to 16 bytes at p (n >= 1 of them valid) as 4 little-endian words, the
// bytes past n zero.  Only 4-byte-aligned dwords holding at least one valid
// byte are read: such a dword never leaves the page its valid byte is on.
__device__ __forceinline__ void load16(const uint8_t* p, unsigned n, uint32_t w[4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    const unsigned sh = (unsigned)(a & 3) * 8;
    const unsigned last = ((unsigned)(a & 3) + n - 1) >> 2;
    uint32_t d[5];
#pragma unroll
    for (unsigned k = 0; k < 5; ++k) d[k] = q[k < last ? k : last];
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const uint32_t v = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);
        const int vb = (int)n - 4 * (int)k;
        w[k] = vb >= 4 ? v : (vb <= 0 ? 0u : v & ((1u << (8 * vb)) - 1u));
    }
}

// lorawan.cpp:35-98 for one frame of `len` bytes, which load(off, have, m)
// hands over 16 at a time, in order: bytes off .. off + have - 1 (1 <= have <=
// 16, off a multiple of 16) as load16 gives them.
template <class Load>
__device__ uint32_t frame_mic_from(const Tab& tb, const uint32_t key[4], bool uplink, uint32_t devaddr,
                                   uint32_t fcnt, uint32_t len, Load load) {
    uint32_t rk[44];
    expand_key(tb, key, rk);
    uint32_t K1[4] = {0, 0, 0, 0}, K2[4];
    encrypt(tb, rk, K1);  // L = E_K(0)
    cmac_double(K1, K1);
    cmac_double(K1, K2);
    // B0 (lorawan.cpp:46-58), bytes 4j..4j+3 of the block in word j
    uint32_t X[4] = {0x49u, (uplink ? 0u : 1u) << 8 | (devaddr & 0xFFFFu) << 16,
                     (devaddr >> 16) | (fcnt & 0xFFFFu) << 16,
                     (fcnt >> 16) | ((len >> 8) & 0xFFu) << 16 | (len & 0xFFu) << 24};
    const uint32_t total = len + 16, nblk = (total + 15) / 16;
    if (nblk == 1) {  // B0 is also the last block (len == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) X[j] ^= K1[j];
        encrypt(tb, rk, X);
        return X[0];
    }
    encrypt(tb, rk, X);
    for (uint32_t b = 1; b < nblk; ++b) {
        const uint32_t have = total - 16 * b < 16 ? total - 16 * b : 16;
        uint32_t m[4];
        load(16 * (b - 1), have, m);
        if (b + 1 == nblk) {
            if (have < 16) m[have >> 2] |= 0x80u << (8 * (have & 3));
            const uint32_t* K = have == 16 ? K1 : K2;
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] ^= K[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) X[j] ^= m[j];
        encrypt(tb, rk, X);
    }
    return X[0];  // tag bytes 0-3, little-endian (lorawan.cpp:94-97)
}

// the same for `len` bytes in memory at `data`
__device__ uint32_t frame_mic(const Tab& tb, const uint32_t key[4], bool uplink, uint32_t devaddr, uint32_t fcnt,
                              const uint8_t* data, uint32_t len) {
    return frame_mic_from(tb, key, uplink, devaddr, fcnt, len,
                          [data](uint32_t off, uint32_t have, uint32_t m[4]) { load16(data + off, have, m); });
}

__device__ __forceinline__ void load_key(const uint8_t* keys, uint32_t idx, uint32_t k[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + 16ull * idx);
    k[0] = v.x, k[1] = v.y, k[2] = v.z, k[3] = v.w;
}

__device__ __forceinline__ Tab lane_tab(const uint32_t* lds) { return Tab{lds + (threadIdx.x & (kCopies - 1))}; }

__global__ void __launch_bounds__(kThreads) k_lw_mic(uint8_t* bytes, const lphy_lorawan_desc* desc,
                                                     unsigned long long frames, const uint8_t* keys,
                                                     unsigned long long nkeys, uint32_t* mic, unsigned flags) {
    extern __shared__ uint32_t lds[];
    build_table(lds);
    const Tab tb = lane_tab(lds);
    for (unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; f < frames;
         f += (unsigned long long)gridDim.x * blockDim.x) {
        const lphy_lorawan_desc d = desc[f];
        if (d.key >= nkeys) {  // no such key: MIC 0, nothing appended
            if (mic) mic[f] = 0;
            continue;
        }
        uint32_t k[4];
        load_key(keys, d.key, k);
        uint8_t* data = bytes + d.offset;
        const uint32_t m = frame_mic(tb, k, d.uplink != 0, d.devaddr, d.fcnt, data, d.len);
        if (mic) mic[f] = m;
        if (flags & LPHY_LW_APPEND) {
#pragma unroll
            for (int j = 0; j < 4; ++j) data[d.len + j] = (uint8_t)(m >> (8 * j));
        }
    }
}

// k_lw_build: one frame of the table per thread.  The frame is handed to the
// CMAC 16 bytes at a time as it is gathered (the 8 header bytes from the
// record, then FOpts and FRMPayload from src through load16), and every block
// is stored on its way through; the MIC follows.  d_bytes gets byte stores
// only: a frame starts and ends at any byte, and the dwords at its ends belong
// partly to neighbours other threads write at the same time.
__global__ void __launch_bounds__(kThreads) k_lw_build(const uint8_t* src, const lphy_lorawan_tx* tx,
                                                       const lphy_ragged_desc* desc, unsigned long long frames,
                                                       unsigned long long step, const uint8_t* keys,
                                                       unsigned long long nkeys, uint8_t* bytes, uint16_t* syms,
                                                       int32_t* status) {
    extern __shared__ uint32_t lds[];
    build_table(lds);
    const Tab tb = lane_tab(lds);
    for (unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; f < frames;
         f += (unsigned long long)gridDim.x * blockDim.x) {
        const uint4* tp = reinterpret_cast<const uint4*>(tx + f);
        const uint4 a = tp[0], b = tp[1];
        const unsigned long long src_offset = a.x | (unsigned long long)a.y << 32;
        const uint32_t devaddr = a.z, key = a.w, payload_len = b.x;
        const uint32_t fcnt = b.y & 0xFFFFu, mtype = (b.y >> 16) & 0xFFu, major = b.y >> 24;
        const uint32_t fctrl = b.z & 0xFFu, fol = (b.z >> 8) & 0xFFu;
        const unsigned long long samples = desc[f].samples, sym_offset = desc[f].sym_offset;
        const unsigned long long L = lw_tx_len(fol, payload_len);
        if (fol > 15 || mtype > 7) {
            status[f] = -EINVAL;
        } else if (key >= nkeys) {
            status[f] = -ENOKEY;
        } else if (samples >= kRaggedMaxSamples || L != lw_slot_bytes(samples, step)) {
            status[f] = -ERANGE;
        } else {  // L < 2^30
            uint8_t* dst = bytes + sym_offset / 2;
            uint16_t* so = syms ? syms + sym_offset : nullptr;
            const bool pair = (sym_offset & 1) == 0;  // a symbol pair is an aligned dword of the slot
            // `n` bytes of w to the frame at byte `off`, and their symbols (LoRaEncoder.cpp:6-18)
            auto put = [&](uint32_t off, uint32_t n, const uint32_t w[4]) {
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    if (i >= n) continue;
                    const uint32_t v = byte_of(w[i >> 2], i & 3);
                    dst[off + i] = (uint8_t)v;
                    if (so) {
                        const uint32_t e = lw_encode_byte(v);
                        uint16_t* p = so + 2ull * (off + i);
                        if (pair) *reinterpret_cast<uint32_t*>(p) = e;
                        else p[0] = (uint16_t)e, p[1] = (uint16_t)(e >> 16);
                    }
                }
            };
            const uint32_t h0 = (mtype << 5 | (major & 3)) | devaddr << 8;
            const uint32_t h1 = devaddr >> 24 | ((fctrl & 0xF0) | fol) << 8 | fcnt << 16;
            const uint8_t* body = src + src_offset;
            uint32_t k[4];
            load_key(keys, key, k);
            const uint32_t m = frame_mic_from(tb, k, (mtype & 1) == 0, devaddr, fcnt, (uint32_t)L - 4,
                                              [&](uint32_t off, uint32_t have, uint32_t w[4]) {
                                                  if (off) {
                                                      load16(body + (off - 8), have, w);
                                                  } else {  // the header, then the first 8 bytes of the body
                                                      uint32_t t[4] = {0, 0, 0, 0};
                                                      if (have > 8) load16(body, have - 8, t);
                                                      w[0] = h0, w[1] = h1, w[2] = t[0], w[3] = t[1];
                                                  }
                                                  put(off, have, w);
                                              });
            const uint32_t mw[4] = {m, 0, 0, 0};
            put((uint32_t)L - 4, 4, mw);
            status[f] = (int32_t)(2 * L);
        }
    }
}

// What parse_frame reads of a row before the MIC is known (lorawan.cpp:152-158).
struct RowHead {
    uint32_t mhdr, devaddr, fctrl, fcnt, mic;
};

__device__ __forceinline__ RowHead row_head(const uint8_t* row, uint32_t len) {
    uint32_t h[4], t[4];
    load16(row, 8, h);
    load16(row + len - 4, 4, t);
    return RowHead{h[0] & 0xFF, (h[0] >> 8) | (h[1] << 24), (h[1] >> 8) & 0xFF, h[1] >> 16, t[0]};
}

__device__ __forceinline__ uint32_t row_mic(const Tab& tb, const uint8_t* keys, uint32_t kidx, const RowHead& h,
                                            const uint8_t* row, uint32_t len) {
    uint32_t k[4];
    load_key(keys, kidx, k);
    return frame_mic(tb, k, ((h.mhdr >> 5) & 1) == 0, h.devaddr, h.fcnt, row, len - 4);
}

// The header fields and the carried MIC of the record.
__device__ __forceinline__ void row_fields(const RowHead& h, uint32_t rec[8]) {
    rec[1] = h.devaddr, rec[2] = h.mic;
    rec[6] = h.fcnt | h.mhdr << 16 | h.fctrl << 24;
    rec[7] = h.fctrl & 0x0F;
}

// The rest once the MIC is computed (lorawan.cpp:161-176).
__device__ __forceinline__ void row_verdict(const RowHead& h, uint32_t calc, uint32_t len, uint32_t rec[8]) {
    const uint32_t fol = h.fctrl & 0x0F;
    row_fields(h, rec);
    rec[3] = calc;
    if (h.mic != calc) {
        rec[0] = (uint32_t)-EINVAL;
    } else if (8 + fol > len - 4) {
        rec[0] = (uint32_t)-ERANGE;
    } else {
        rec[4] = 8 + fol;
        rec[5] = len - 12 - fol;
        rec[0] = rec[5];
    }
}

__device__ __forceinline__ void store_record(lphy_lorawan_frame* out, const uint32_t rec[8]) {
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    o[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
}

// lorawan.cpp:150-176 on one row of decoded bytes.
__global__ void __launch_bounds__(kThreads) k_lw_parse(const uint8_t* bytes, unsigned long long frames,
                                                       unsigned long long stride, const uint32_t* lens,
                                                       uint32_t len0, const uint8_t* keys,
                                                       unsigned long long nkeys, const uint32_t* key_index,
                                                       lphy_lorawan_frame* out) {
    extern __shared__ uint32_t lds[];
    build_table(lds);
    const Tab tb = lane_tab(lds);
    for (unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; f < frames;
         f += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t len = lens ? lens[f] : len0;
        const uint8_t* row = bytes + f * stride;
        uint32_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t kidx = key_index ? key_index[f] : 0u;
        // a row length past the row (or past the 16-bit record fields) would
        // read beyond the row: -ERANGE, nothing read
        if (len < 12 || len > stride || len > 65535u) {
            rec[0] = (uint32_t)-ERANGE;
        } else if (kidx >= nkeys) {
            rec[0] = (uint32_t)-ENOKEY;
        } else {
            const RowHead h = row_head(row, len);
            row_verdict(h, row_mic(tb, keys, kidx, h, row, len), len, rec);
        }
        store_record(out + f, rec);
    }
}

// The same on the rows lphy_hip_demod_ragged left: row f is the decoded bytes
// of the frame's output symbols at sym_offset / 2.  The key is key_index[f],
// key 0, or - with a session table - the first of the up to kLwMaxCandidates
// records with the row's DevAddr whose MIC matches.
__global__ void __launch_bounds__(kThreads) k_lw_parse_ragged(
    const uint8_t* bytes, const lphy_ragged_desc* desc, unsigned long long frames, unsigned long long step, int mode,
    const lphy_frame_meta* meta, const uint8_t* keys, unsigned long long nkeys, const uint32_t* key_index,
    const lphy_lorawan_session* sessions, unsigned long long nsessions, lphy_lorawan_frame* out,
    uint32_t* key_used) {
    extern __shared__ uint32_t lds[];
    build_table(lds);
    const Tab tb = lane_tab(lds);
    for (unsigned long long f = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; f < frames;
         f += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long samples = desc[f].samples, sym_offset = desc[f].sym_offset;
        uint32_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t used = kLwNoKey;
        const unsigned long long len64 = samples < kRaggedMaxSamples ? ragged_out_syms(samples / step, mode) / 2 : 0;
        const uint32_t kidx = key_index ? key_index[f] : 0u;
        int32_t st = 0;
        if (samples >= kRaggedMaxSamples) {
            rec[0] = (uint32_t)-ERANGE;
        } else if (meta && (st = meta[f].status) != 0) {  // decode's error (lorawan.cpp:149)
            rec[0] = (uint32_t)st;
        } else if (len64 < 12 || len64 > 65535u) {
            rec[0] = (uint32_t)-ERANGE;
        } else if (!sessions && kidx >= nkeys) {
            rec[0] = (uint32_t)-ENOKEY;
        } else {
            const uint32_t len = (uint32_t)len64;
            const uint8_t* row = bytes + sym_offset / 2;
            const RowHead h = row_head(row, len);
            // the candidates: the one key, or the records with the row's DevAddr
            const unsigned long long first = sessions ? lw_lower_bound(sessions, nsessions, h.devaddr) : 0;
            uint32_t calc = 0;
            for (unsigned c = 0; c < (sessions ? kLwMaxCandidates : 1u); ++c) {
                uint32_t k = kidx;
                if (sessions) {
                    if (first + c >= nsessions || sessions[first + c].devaddr != h.devaddr) break;
                    k = sessions[first + c].key;
                    if (k >= nkeys) continue;
                }
                const uint32_t m = row_mic(tb, keys, k, h, row, len);
                if (used == kLwNoKey || m == h.mic) used = k, calc = m;  // the first, then the match
                if (m == h.mic) break;
            }
            if (used == kLwNoKey) {
                row_fields(h, rec);
                rec[0] = (uint32_t)-ENOKEY;
            } else {
                row_verdict(h, calc, len, rec);
            }
        }
        store_record(out + f, rec);
        if (key_used) key_used[f] = used;
    }
}

// ---------------------------------------------------- FRMPayload cipher
// The n (1..16) low bytes of w to p.  A range's neighbours are written by other
// lanes at the same time, so nothing is read and written back: the bytes in
// front of the first aligned dword and behind the last whole one go out as
// bytes, the aligned dwords the block fills as dwords.
__device__ __forceinline__ void store16(uint8_t* p, unsigned n, const uint32_t w[4]) {
    const unsigned lead = (unsigned)(-reinterpret_cast<uintptr_t>(p)) & 3;
    const unsigned head = lead < n ? lead : n;
    const unsigned whole = (n - head) >> 2, tail = (n - head) & 3;
#pragma unroll
    for (unsigned i = 0; i < 3; ++i)
        if (i < head) p[i] = (uint8_t)byte_of(w[0], i);
    uint32_t* q = reinterpret_cast<uint32_t*>(p + head);
    const uint32_t e[5] = {w[0], w[1], w[2], w[3], 0};
    uint32_t last = 0;  // the bytes behind the whole dwords
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const uint32_t v = __builtin_amdgcn_alignbit(e[k + 1], e[k], 8 * head);
        if (k < whole) q[k] = v;
        if (k == whole) last = v;
    }
    uint8_t* t = reinterpret_cast<uint8_t*>(q + whole);
#pragma unroll
    for (unsigned i = 0; i < 3; ++i)
        if (i < tail) t[i] = (uint8_t)byte_of(last, i);
}

// The three forms of the cipher resolve record f to a job
// (lphy_lorawan_ragged.h); every lane of a group resolves the same one.
struct CryptBatch {
    const lphy_lorawan_desc* desc;
    __device__ LwCryptJob operator()(unsigned long long f, unsigned long long nkeys) const {
        return lw_crypt_job_batch(desc[f], nkeys);
    }
};

struct CryptTx {
    const lphy_lorawan_tx* tx;
    unsigned skip;
    __device__ LwCryptJob operator()(unsigned long long f, unsigned long long nkeys) const {
        return lw_crypt_job_tx(tx[f], nkeys, skip);
    }
};

struct CryptRx {
    const lphy_ragged_desc* desc;
    const lphy_lorawan_frame* parsed;
    const uint32_t* key_used;
    unsigned long long step;
    int mode;
    unsigned skip;
    __device__ LwCryptJob operator()(unsigned long long f, unsigned long long nkeys) const {
        return lw_crypt_job_rx(desc[f], parsed[f], key_used ? key_used[f] : 0u, step, mode, nkeys, skip);
    }
};

// Lanes of a job: lane g of the group makes keystream blocks g + 1, g + 1 + G, ...
// G = 2 by measurement (tools/lorawan_crypt_bench.py): every lane
// with a block pays a key expansion, about one more block's worth of dependent
// table reads, so wider groups lose on the 1..16 blocks LoRaWAN payloads have.
#ifndef LPHY_LW_CRYPT_G
#define LPHY_LW_CRYPT_G 2
#endif
constexpr unsigned kCryptG = LPHY_LW_CRYPT_G;
static_assert(kCryptG >= 1 && kCryptG <= 32 && (kCryptG & (kCryptG - 1)) == 0, "a power of two dividing 32");

// k_lw_crypt: the keystream blocks of a range are independent, so G
// consecutive lanes share a job and each lane that has a block expands the key
// for itself.  The table replica is still threadIdx.x & 31: 32 different banks
// per ds_read_b32 group whatever G is.
template <class Front>
__global__ void __launch_bounds__(kThreads) k_lw_crypt(uint8_t* bytes, Front front, unsigned long long jobs,
                                                       const uint8_t* keys, unsigned long long nkeys,
                                                       int32_t* status) {
    extern __shared__ uint32_t lds[];
    build_table(lds);
    const Tab tb = lane_tab(lds);
    constexpr unsigned per = kThreads / kCryptG;  // jobs of a workgroup per trip
    const unsigned g = threadIdx.x % kCryptG;
    for (unsigned long long f = (unsigned long long)blockIdx.x * per + threadIdx.x / kCryptG; f < jobs;
         f += (unsigned long long)gridDim.x * per) {
        const LwCryptJob job = front(f, nkeys);
        if (status && g == 0) status[f] = job.status;
        const uint32_t nblk = job.status ? 0u : (job.len + 15) / 16;
        if (g >= nblk) continue;
        uint32_t k[4], rk[44];
        load_key(keys, job.key, k);
        expand_key(tb, k, rk);
        uint8_t* data = bytes + job.offset;
        for (uint32_t b = g; b < nblk; b += kCryptG) {
            const uint32_t have = job.len - 16 * b < 16 ? job.len - 16 * b : 16;
            uint32_t s[4], w[4];
            lw_crypt_block(job.uplink, job.devaddr, job.fcnt, b + 1, s);
            load16(data + 16 * b, have, w);  // in flight during the rounds
            encrypt(tb, rk, s);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] ^= s[j];
            store16(data + 16 * b, have, w);
        }
    }
}

unsigned grid_for(unsigned long long frames) {
    const unsigned long long b = (frames + kThreads - 1) / kThreads;
    return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

constexpr size_t kLds = 256 * kCopies * sizeof(uint32_t);  // 32 KiB

// One launch of k_lw_crypt for `jobs` records (0 < jobs < 2^31) of a front end.
template <class Front>
int launch_crypt(uint8_t* bytes, Front front, size_t jobs, const uint8_t* keys, size_t nkeys, int32_t* status,
                 void* stream) {
    hipLaunchKernelGGL(k_lw_crypt<Front>, dim3(grid_for((unsigned long long)jobs * kCryptG)), dim3(kThreads), kLds,
                       (hipStream_t)stream, bytes, front, (unsigned long long)jobs, keys, (unsigned long long)nkeys,
                       status);
    LW_OK(hipGetLastError());
    return 0;
}

// The staging buffer of the host forms on `device`, at least `need` bytes; the
// device made current.  The caller holds g_stage_mu, which serialises them.
std::mutex g_stage_mu;

int host_stage(int device, size_t need, uint8_t** base) {
    struct Stage {
        void* p = nullptr;
        size_t bytes = 0;
    };
    static std::map<int, Stage> stages;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
    LW_OK(hipSetDevice(device));
    Stage& s = stages[device];
    if (s.bytes < need) {
        if (s.p) (void)hipFree(s.p);
        s.p = nullptr;
        s.bytes = 0;
        LW_OK(hipMalloc(&s.p, need < 4096 ? 4096 : need));
        s.bytes = need < 4096 ? 4096 : need;
    }
    *base = static_cast<uint8_t*>(s.p);
    return 0;
}

}  // namespace

static_assert(sizeof(lphy_lorawan_desc) == 32, "descriptor layout");
static_assert(sizeof(lphy_lorawan_frame) == 32, "record layout");
static_assert(sizeof(lphy_lorawan_tx) == 32 && sizeof(lphy_lorawan_session) == 8, "ragged record layouts");

extern "C" {

int lphy_hip_lorawan_mic_batch(uint8_t* d_bytes, const lphy_lorawan_desc* d_desc, size_t frames,
                               const uint8_t* d_keys, size_t nkeys, uint32_t* d_mic, unsigned flags,
                               void* stream) {
    if (!frames) return 0;
    if (!d_bytes || !d_desc || !d_keys || !nkeys || (!d_mic && !(flags & LPHY_LW_APPEND))) return -EINVAL;
    if (flags & ~LPHY_LW_APPEND) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_desc) & 15) return -EINVAL;
    hipLaunchKernelGGL(k_lw_mic, dim3(grid_for(frames)), dim3(kThreads), kLds, (hipStream_t)stream, d_bytes,
                       d_desc, (unsigned long long)frames, d_keys, (unsigned long long)nkeys, d_mic, flags);
    LW_OK(hipGetLastError());
    return 0;
}

int lphy_hip_lorawan_parse_batch(const uint8_t* d_bytes, size_t frames, size_t stride,
                                 const uint32_t* d_lens, size_t len, const uint8_t* d_keys, size_t nkeys,
                                 const uint32_t* d_key_index, lphy_lorawan_frame* d_out, void* stream) {
    if (!frames) return 0;
    if (!d_bytes || !d_keys || !nkeys || !d_out) return -EINVAL;
    if (!d_lens && (len > stride || len > 65535)) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_out) & 15) return -EINVAL;
    hipLaunchKernelGGL(k_lw_parse, dim3(grid_for(frames)), dim3(kThreads), kLds, (hipStream_t)stream, d_bytes,
                       (unsigned long long)frames, (unsigned long long)stride, d_lens, (uint32_t)len, d_keys,
                       (unsigned long long)nkeys, d_key_index, d_out);
    LW_OK(hipGetLastError());
    return 0;
}

int lphy_hip_lorawan_build_ragged(const uint8_t* d_src, const lphy_lorawan_tx* d_tx, const lphy_ragged_desc* d_desc,
                                  size_t frames, size_t symbol_samples, const uint8_t* d_keys, size_t nkeys,
                                  uint8_t* d_bytes, uint16_t* d_syms_out, int32_t* d_status, void* stream) {
    if (!frames) return 0;
    if (!d_src || !d_tx || !d_desc || !d_keys || !d_bytes || !d_status || !symbol_samples || !nkeys) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_tx) & 15) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    hipLaunchKernelGGL(k_lw_build, dim3(grid_for(frames)), dim3(kThreads), kLds, (hipStream_t)stream, d_src, d_tx,
                       d_desc, (unsigned long long)frames, (unsigned long long)symbol_samples, d_keys,
                       (unsigned long long)nkeys, d_bytes, d_syms_out, d_status);
    LW_OK(hipGetLastError());
    return 0;
}

int lphy_hip_lorawan_parse_ragged(const uint8_t* d_bytes, const lphy_ragged_desc* d_desc, size_t frames,
                                  size_t symbol_samples, int mode, const lphy_frame_meta* d_meta,
                                  const uint8_t* d_keys, size_t nkeys, const uint32_t* d_key_index,
                                  const lphy_lorawan_session* d_sessions, size_t nsessions,
                                  lphy_lorawan_frame* d_out, uint32_t* d_key_used, void* stream) {
    if (!frames) return 0;
    if (!d_bytes || !d_desc || !d_keys || !d_out || !nkeys || !symbol_samples) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_out) & 15) return -EINVAL;
    if ((d_key_index && d_sessions) || (d_sessions && !nsessions)) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    hipLaunchKernelGGL(k_lw_parse_ragged, dim3(grid_for(frames)), dim3(kThreads), kLds, (hipStream_t)stream, d_bytes,
                       d_desc, (unsigned long long)frames, (unsigned long long)symbol_samples, mode, d_meta, d_keys,
                       (unsigned long long)nkeys, d_key_index, d_sessions,
                       (unsigned long long)(d_sessions ? nsessions : 0), d_out, d_key_used);
    LW_OK(hipGetLastError());
    return 0;
}

int lphy_hip_lorawan_sessions_check(const lphy_lorawan_session* h_sessions, size_t n) {
    return lw_sessions_check(h_sessions, n);
}

int lphy_hip_lorawan_crypt_batch(uint8_t* d_bytes, const lphy_lorawan_desc* d_desc, size_t jobs,
                                 const uint8_t* d_keys, size_t nkeys, int32_t* d_status, void* stream) {
    if (!jobs) return 0;
    if (!d_bytes || !d_desc || !d_keys || !nkeys) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_desc) & 15) return -EINVAL;
    if (jobs > kRaggedMaxFrames) return -ERANGE;
    return launch_crypt(d_bytes, CryptBatch{d_desc}, jobs, d_keys, nkeys, d_status, stream);
}

int lphy_hip_lorawan_crypt_tx_ragged(uint8_t* d_src, const lphy_lorawan_tx* d_tx, size_t frames,
                                     const uint8_t* d_keys, size_t nkeys, unsigned skip, int32_t* d_status,
                                     void* stream) {
    if (!frames) return 0;
    if (!d_src || !d_tx || !d_keys || !nkeys || skip > 1) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_tx) & 15) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    return launch_crypt(d_src, CryptTx{d_tx, skip}, frames, d_keys, nkeys, d_status, stream);
}

int lphy_hip_lorawan_crypt_rx_ragged(uint8_t* d_bytes, const lphy_ragged_desc* d_desc,
                                     const lphy_lorawan_frame* d_parsed, const uint32_t* d_key_used, size_t frames,
                                     size_t symbol_samples, int mode, const uint8_t* d_keys, size_t nkeys,
                                     unsigned skip, int32_t* d_status, void* stream) {
    if (!frames) return 0;
    if (!d_bytes || !d_desc || !d_parsed || !d_keys || !nkeys || !symbol_samples || skip > 1) return -EINVAL;
    if (mode < 0 || mode > 2) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15 || reinterpret_cast<uintptr_t>(d_parsed) & 15) return -EINVAL;
    if (frames > kRaggedMaxFrames) return -ERANGE;
    return launch_crypt(d_bytes, CryptRx{d_desc, d_parsed, d_key_used, (unsigned long long)symbol_samples, mode, skip},
                        frames, d_keys, nkeys, d_status, stream);
}

int lphy_hip_lorawan_mic_host(int device, const uint8_t key[16], int uplink, uint32_t devaddr, uint32_t fcnt,
                              const uint8_t* data, size_t len, uint32_t* mic) {
    if (!key || !mic || (len && !data) || len > 0xFFFFFFFFull - 64) return -EINVAL;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    // [key 16 | desc 32 | mic 4 .. pad to 64 | data]
    uint8_t* base = nullptr;
    if (int rc = host_stage(device, 64 + len + 4, &base)) return rc;
    lphy_lorawan_desc d{};
    d.offset = 64;
    d.len = (uint32_t)len;
    d.devaddr = devaddr;
    d.fcnt = fcnt;
    d.key = 0;
    d.uplink = uplink ? 1u : 0u;
    LW_OK(hipMemcpy(base, key, 16, hipMemcpyHostToDevice));
    LW_OK(hipMemcpy(base + 16, &d, sizeof d, hipMemcpyHostToDevice));
    if (len) LW_OK(hipMemcpy(base + 64, data, len, hipMemcpyHostToDevice));
    const int rc = lphy_hip_lorawan_mic_batch(base, reinterpret_cast<const lphy_lorawan_desc*>(base + 16), 1,
                                              base, 1, reinterpret_cast<uint32_t*>(base + 48), 0, nullptr);
    if (rc) return rc;
    LW_OK(hipDeviceSynchronize());
    LW_OK(hipMemcpy(mic, base + 48, 4, hipMemcpyDeviceToHost));
    return 0;
}

int lphy_hip_lorawan_crypt_host(int device, const uint8_t key[16], int uplink, uint32_t devaddr, uint32_t fcnt,
                                uint8_t* data, size_t len) {
    if (!key || (len && !data)) return -EINVAL;
    if (len > kLwCryptMaxLen) return -ERANGE;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    // [key 16 | desc 32 | status 4 .. pad to 64 | data]
    uint8_t* base = nullptr;
    if (int rc = host_stage(device, 64 + len + 4, &base)) return rc;
    if (!len) return 0;
    lphy_lorawan_desc d{};
    d.offset = 64;
    d.len = (uint32_t)len;
    d.devaddr = devaddr;
    d.fcnt = fcnt;
    d.key = 0;
    d.uplink = uplink ? 1u : 0u;
    LW_OK(hipMemcpy(base, key, 16, hipMemcpyHostToDevice));
    LW_OK(hipMemcpy(base + 16, &d, sizeof d, hipMemcpyHostToDevice));
    LW_OK(hipMemcpy(base + 64, data, len, hipMemcpyHostToDevice));
    const int rc = lphy_hip_lorawan_crypt_batch(base, reinterpret_cast<const lphy_lorawan_desc*>(base + 16), 1, base,
                                                1, reinterpret_cast<int32_t*>(base + 48), nullptr);
    if (rc) return rc;
    LW_OK(hipDeviceSynchronize());
    int32_t st = 0;
    LW_OK(hipMemcpy(&st, base + 48, 4, hipMemcpyDeviceToHost));
    if (st) return st;
    LW_OK(hipMemcpy(data, base + 64, len, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
