// Host-only test library over csrc/lphy_lorawan_ragged.h: what
// lphy_hip_lorawan_tx_layout runs for a context of (sf, osr),
// lphy_hip_lorawan_sessions_check, and the lower-bound search, frame geometry
// and byte encoder the kernels of lphy_lorawan.hip compile from the same
// header (tests/test_lorawan_ragged_cpu.py loads it through ctypes).  With
// -DLW_RAGGED_MAIN it is a stand-alone program over the same helpers, for a
// run under the host sanitizers.
#include "lphy_lorawan_ragged.h"

using namespace lphy;

extern "C" int lw_tx_layout_check(unsigned sf, unsigned osr, const lphy_lorawan_tx* h_tx, size_t frames,
                                  lphy_ragged_desc* h_desc) {
    return lw_tx_layout((uint64_t(1) << sf) * osr, h_tx, frames, h_desc);
}

extern "C" int lw_plain_tx_layout_check(unsigned sf, unsigned osr, const uint64_t* h_len_bytes, size_t frames,
                                        lphy_ragged_desc* h_desc) {
    return tx_layout((uint64_t(1) << sf) * osr, h_len_bytes, frames, h_desc);
}

extern "C" int lw_sessions_check_check(const lphy_lorawan_session* s, size_t n) { return lw_sessions_check(s, n); }

extern "C" void lw_lower_bound_check(const lphy_lorawan_session* s, size_t n, const uint32_t* devaddr, size_t queries,
                                     uint64_t* out) {
    for (size_t i = 0; i < queries; ++i) out[i] = lw_lower_bound(s, n, devaddr[i]);
}

extern "C" uint64_t lw_slot_bytes_check(uint64_t samples, uint64_t step) { return lw_slot_bytes(samples, step); }

// the two symbols of every byte value: out[2 b], out[2 b + 1]
extern "C" void lw_encode_bytes_check(uint16_t* out) {
    for (uint32_t b = 0; b < 256; ++b) {
        out[2 * b] = (uint16_t)lw_encode_byte(b);
        out[2 * b + 1] = (uint16_t)(lw_encode_byte(b) >> 16);
    }
}

#ifdef LW_RAGGED_MAIN
#include <cstdio>

#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                          \
        }                                                      \
    } while (0)

int main() {
    // tx_layout on L = 12 + fopts_len + payload_len; heap tables, so that a read
    // or write past either end is the sanitizer's to see
    const size_t nf = 300;
    std::vector<lphy_lorawan_tx> tx(nf);
    std::vector<uint64_t> len(nf);
    for (size_t f = 0; f < nf; ++f) {
        tx[f] = lphy_lorawan_tx{};
        tx[f].fopts_len = (uint8_t)(f % 16);
        tx[f].payload_len = (uint32_t)(f * 7 % 223);
        len[f] = 12 + tx[f].fopts_len + tx[f].payload_len;
    }
    std::vector<lphy_ragged_desc> a(nf + 1), b(nf + 1);
    EXPECT(lw_tx_layout(128, tx.data(), nf, a.data()) == 0);
    EXPECT(tx_layout(128, len.data(), nf, b.data()) == 0);
    for (size_t f = 0; f <= nf; ++f)
        EXPECT(a[f].iq_offset == b[f].iq_offset && a[f].samples == b[f].samples && a[f].sym_offset == b[f].sym_offset &&
               a[f].unit_offset == b[f].unit_offset);
    for (size_t f = 0; f < nf; ++f) EXPECT(lw_slot_bytes(a[f].samples, 128) == len[f]);
    std::vector<lphy_ragged_desc> one(1);
    EXPECT(lw_tx_layout(256, nullptr, 0, one.data()) == 0 && one[0].unit_offset == 0);
    EXPECT(lw_tx_layout(128, tx.data(), nf, nullptr) == -EINVAL);
    EXPECT(lw_tx_layout(128, nullptr, 1, one.data()) == -EINVAL);
    tx[nf - 1].fopts_len = 16;
    EXPECT(lw_tx_layout(128, tx.data(), nf, a.data()) == -EINVAL);
    tx[nf - 1].fopts_len = 0;
    tx[nf - 1].payload_len = 0xFFFFFFFFu;
    EXPECT(lw_tx_layout(128, tx.data(), nf, a.data()) == -ERANGE);

    // sessions_check and the lower bound on exactly-sized tables
    for (size_t n = 0; n <= 40; ++n) {
        std::vector<lphy_lorawan_session> s(n);
        for (size_t i = 0; i < n; ++i) s[i] = lphy_lorawan_session{(uint32_t)(i / 9 * 5), (uint32_t)i};
        EXPECT(lw_sessions_check(n ? s.data() : nullptr, n) == 0);
        for (uint32_t q = 0; q < 30; ++q) {
            size_t want = 0;
            while (want < n && s[want].devaddr < q) ++want;
            EXPECT(lw_lower_bound(s.data(), n, q) == want);
        }
        EXPECT(lw_lower_bound(s.data(), n, 0xFFFFFFFFu) == n);
        if (n >= 2) {
            s[n - 1].devaddr = 0;
            s[0].devaddr = 0xFFFFFFFFu;
            EXPECT(lw_sessions_check(s.data(), n) == -EINVAL);
            EXPECT(lw_lower_bound(s.data(), n, 7) <= n);  // an unsorted table stays inside
        }
    }
    EXPECT(lw_sessions_check(nullptr, 3) == -EINVAL);
    EXPECT(lw_encode_byte(0x00) == 0 && (lw_encode_byte(0xF0) & 0xFFFF) == 0xFF);
    std::printf("lorawan_ragged_check: ok\n");
    return 0;
}
#endif
