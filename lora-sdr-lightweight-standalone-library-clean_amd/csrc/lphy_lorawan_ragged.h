// lphy_lorawan_ragged.h — what the LoRaWAN calls on a ragged table
// (lphy_hip_lorawan_build_ragged, lphy_hip_lorawan_parse_ragged) share between
// the kernels of lphy_lorawan.hip and the host: the frame geometry, the
// lower-bound search of the session table, encodeHamming84sx of a byte, the
// payload cipher's A_i block and the front ends that resolve a record to a
// cipher job (lphy_hip_lorawan_crypt_*), and the two host-only helpers
// (lphy_hip_lorawan_tx_layout, lphy_hip_lorawan_sessions_check).  Plain C++
// with LPHY_RG_HD (lphy_ragged_layout.h) in front of what the kernels call
// too, so the CPU tests compile it alone (tests/cpp/lorawan_ragged_check.cpp,
// tests/cpp/lorawan_crypt_check.cpp).
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "lphy_ragged_layout.h"

namespace lphy {

constexpr unsigned kLwMaxCandidates = 8;  // session records tried per frame
constexpr uint32_t kLwNoKey = 0xFFFFFFFFu;

// MHDR .. MIC of a frame to build: 12 + FOpts + FRMPayload (lorawan.cpp:108)
LPHY_RG_HD constexpr uint64_t lw_tx_len(uint32_t fopts_len, uint32_t payload_len) {
    return 12u + uint64_t(fopts_len) + payload_len;
}

// bytes a frame of `samples` samples carries on air: its data symbols / 2
LPHY_RG_HD constexpr uint64_t lw_slot_bytes(uint64_t samples, uint64_t step) {
    return ragged_out_syms(samples / step, LPHY_MODE_DEMODULATE) / 2;
}

// first record whose devaddr is not below `devaddr` (n when there is none) of
// a table sorted by devaddr ascending.  At most 64 steps whatever the table
// holds, sorted or not.
LPHY_RG_HD inline size_t lw_lower_bound(const lphy_lorawan_session* s, size_t n, uint32_t devaddr) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (s[mid].devaddr < devaddr) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// encodeHamming84sx (LoRaCodes.hpp:229-242) of both nibbles of a byte, as
// lora_encode orders them (LoRaEncoder.cpp:6-18): the high nibble's symbol in
// bits 0-15, the low nibble's in bits 16-31
LPHY_RG_HD constexpr uint32_t lw_enc84(uint32_t x) {
    return (x & 0xF) | (((x ^ x >> 1 ^ x >> 2) & 1) << 4) | (((x >> 1 ^ x >> 2 ^ x >> 3) & 1) << 5) |
           (((x ^ x >> 1 ^ x >> 3) & 1) << 6) | (((x ^ x >> 2 ^ x >> 3) & 1) << 7);
}
LPHY_RG_HD constexpr uint32_t lw_encode_byte(uint32_t b) { return lw_enc84((b >> 4) & 0xF) | lw_enc84(b & 0xF) << 16; }

// ------------------------------------------------- FRMPayload cipher
// LoRaWAN 1.0.x 4.3.3: the range is XORed with S_1 | S_2 | ..., S_i =
// AES128(K, A_i).  i is one byte, so a range has at most 255 blocks.
constexpr uint32_t kLwCryptMaxLen = 255u * 16u;

// A_i as four little-endian words (bytes 4j .. 4j + 3 in word j): B0 of
// compute_mic (lorawan.cpp:46-58) with 0x49 -> 0x01 and byte 15 = i
LPHY_RG_HD inline void lw_crypt_block(bool uplink, uint32_t devaddr, uint32_t fcnt, uint32_t i, uint32_t a[4]) {
    a[0] = 0x01u;
    a[1] = (uplink ? 0u : 1u) << 8 | (devaddr & 0xFFFFu) << 16;
    a[2] = devaddr >> 16 | (fcnt & 0xFFFFu) << 16;
    a[3] = fcnt >> 16 | (i & 0xFFu) << 24;
}

// What a front end of the cipher kernel resolves a record to: `len` bytes at
// byte `offset` of the buffer, or a status that refuses the job.
struct LwCryptJob {
    uint64_t offset;
    uint32_t len, devaddr, fcnt, key;
    bool uplink;
    int32_t status;
};

LPHY_RG_HD inline LwCryptJob lw_crypt_refuse(int32_t status) { return LwCryptJob{0, 0, 0, 0, 0, false, status}; }

// lphy_hip_lorawan_crypt_batch
LPHY_RG_HD inline LwCryptJob lw_crypt_job_batch(const lphy_lorawan_desc& d, uint64_t nkeys) {
    if (d.key >= nkeys) return lw_crypt_refuse(-ENOKEY);
    if (d.len > kLwCryptMaxLen) return lw_crypt_refuse(-ERANGE);
    return LwCryptJob{d.offset, d.len, d.devaddr, d.fcnt, d.key, d.uplink != 0, 0};
}

// lphy_hip_lorawan_crypt_tx_ragged: FRMPayload behind FOpts at src_offset,
// the checks in lphy_hip_lorawan_build_ragged's order
LPHY_RG_HD inline LwCryptJob lw_crypt_job_tx(const lphy_lorawan_tx& t, uint64_t nkeys, uint32_t skip) {
    if (t.fopts_len > 15 || t.mtype > 7) return lw_crypt_refuse(-EINVAL);
    if (t.key >= nkeys) return lw_crypt_refuse(-ENOKEY);
    const uint32_t len = t.payload_len > skip ? t.payload_len - skip : 0;
    if (len > kLwCryptMaxLen) return lw_crypt_refuse(-ERANGE);
    return LwCryptJob{t.src_offset + t.fopts_len + skip, len, t.devaddr, t.fcnt, t.key, (t.mtype & 1) == 0, 0};
}

// lphy_hip_lorawan_crypt_rx_ragged: FRMPayload of the row
// lphy_hip_lorawan_parse_ragged parsed (the same row length), `key` what
// d_key_used holds for the frame (0 without it)
LPHY_RG_HD inline LwCryptJob lw_crypt_job_rx(const lphy_ragged_desc& d, const lphy_lorawan_frame& r, uint32_t key,
                                             uint64_t step, int mode, uint64_t nkeys, uint32_t skip) {
    if (d.samples >= kRaggedMaxSamples) return lw_crypt_refuse(-ERANGE);
    if (r.status < 0) return lw_crypt_refuse(r.status);
    const uint64_t row = ragged_out_syms(d.samples / step, mode) / 2;
    if (uint64_t(r.payload_offset) + r.payload_len + 4 > row || r.payload_offset < 8) return lw_crypt_refuse(-EINVAL);
    if (key == kLwNoKey || key >= nkeys) return lw_crypt_refuse(-ENOKEY);
    const uint32_t len = r.payload_len > skip ? r.payload_len - skip : 0;
    if (len > kLwCryptMaxLen) return lw_crypt_refuse(-ERANGE);
    return LwCryptJob{d.sym_offset / 2 + r.payload_offset + skip, len, r.devaddr, r.fcnt, key,
                      ((r.mhdr >> 5) & 1) == 0, 0};
}

// lphy_hip_lorawan_sessions_check
inline int lw_sessions_check(const lphy_lorawan_session* s, size_t n) {
    if (n && !s) return -EINVAL;
    for (size_t i = 1; i < n; ++i)
        if (s[i].devaddr < s[i - 1].devaddr) return -EINVAL;
    return 0;
}

// lphy_hip_lorawan_tx_layout: tx_layout on the frames' lengths
inline int lw_tx_layout(uint64_t step, const lphy_lorawan_tx* h_tx, size_t frames, lphy_ragged_desc* h_desc) {
    if (!h_desc || (frames && !h_tx) || step == 0) return -EINVAL;
    std::vector<uint64_t> len;
    try {
        len.resize(frames);
    } catch (const std::bad_alloc&) {
        return -ENOMEM;
    }
    for (size_t f = 0; f < frames; ++f) {
        if (h_tx[f].fopts_len > 15) return -EINVAL;
        len[f] = lw_tx_len(h_tx[f].fopts_len, h_tx[f].payload_len);
    }
    return tx_layout(step, len.data(), frames, h_desc);
}

}  // namespace lphy
