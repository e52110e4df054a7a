// Host-only test library over the payload-cipher pieces of
// csrc/lphy_lorawan_ragged.h: the A_i block and the three front ends that
// resolve a record to a job or a status, as k_lw_crypt of lphy_lorawan.hip
// compiles them from the same header (tests/test_lorawan_crypt_cpu.py loads it
// through ctypes).  With -DLW_CRYPT_MAIN it is a stand-alone program over the
// same helpers, for a run under the host sanitizers.
#include "lphy_lorawan_ragged.h"

using namespace lphy;

// the 16 bytes of A_i
extern "C" void lw_crypt_block_check(int uplink, uint32_t devaddr, uint32_t fcnt, uint32_t i, uint8_t* out) {
    uint32_t a[4];
    lw_crypt_block(uplink != 0, devaddr, fcnt, i, a);
    for (int j = 0; j < 16; ++j) out[j] = (uint8_t)(a[j / 4] >> (8 * (j % 4)));
}

// out: status, offset, len, devaddr, fcnt, key, uplink
static void put_job(const LwCryptJob& j, int64_t* out) {
    out[0] = j.status, out[1] = (int64_t)j.offset, out[2] = j.len, out[3] = j.devaddr, out[4] = j.fcnt;
    out[5] = j.key, out[6] = j.uplink;
}

extern "C" void lw_crypt_job_batch_check(const lphy_lorawan_desc* d, uint64_t nkeys, int64_t* out) {
    put_job(lw_crypt_job_batch(*d, nkeys), out);
}

extern "C" void lw_crypt_job_tx_check(const lphy_lorawan_tx* t, uint64_t nkeys, uint32_t skip, int64_t* out) {
    put_job(lw_crypt_job_tx(*t, nkeys, skip), out);
}

extern "C" void lw_crypt_job_rx_check(const lphy_ragged_desc* d, const lphy_lorawan_frame* r, uint32_t key,
                                      uint64_t step, int mode, uint64_t nkeys, uint32_t skip, int64_t* out) {
    put_job(lw_crypt_job_rx(*d, *r, key, step, mode, nkeys, skip), out);
}

extern "C" uint32_t lw_crypt_max_len_check() { return kLwCryptMaxLen; }

#ifdef LW_CRYPT_MAIN
#include <cstdio>
#include <memory>

#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                          \
        }                                                      \
    } while (0)

int main() {
    // every record on the heap by itself, so that a read past it is the sanitizer's to see
    for (uint32_t i = 0; i <= 256; ++i) {
        std::unique_ptr<uint32_t[]> a(new uint32_t[4]);
        lw_crypt_block(i & 1, 0x01020304u, 0x0A0B0C0Du, i, a.get());
        EXPECT(a[0] == 1 && a[3] >> 24 == (i & 0xFF) && (a[1] >> 8 & 0xFF) == ((i & 1) ? 0u : 1u));
        EXPECT((a[1] >> 16 | a[2] << 16) == 0x01020304u && (a[2] >> 16 | a[3] << 16) == 0x0A0B0C0Du);
    }
    for (uint32_t len : {0u, 1u, 4080u, 4081u, 0xFFFFFFFFu}) {
        std::unique_ptr<lphy_lorawan_desc> d(new lphy_lorawan_desc{});
        d->offset = 77, d->len = len, d->key = 2, d->uplink = 5;
        const LwCryptJob j = lw_crypt_job_batch(*d, 3);
        EXPECT(j.status == (len > 4080 ? -ERANGE : 0));
        EXPECT(j.status || (j.offset == 77 && j.len == len && j.uplink && j.key == 2));
        EXPECT(lw_crypt_job_batch(*d, 2).status == -ENOKEY);
    }
    for (uint32_t skip = 0; skip < 2; ++skip)
        for (uint32_t pl : {0u, 1u, 2u, 4080u, 4081u, 4082u, 0xFFFFFFFFu}) {
            std::unique_ptr<lphy_lorawan_tx> t(new lphy_lorawan_tx{});
            t->src_offset = uint64_t(1) << 40, t->payload_len = pl, t->fopts_len = 15, t->mtype = 3, t->key = 9;
            t->fcnt = 0xFFFF;
            const LwCryptJob j = lw_crypt_job_tx(*t, 10, skip);
            const uint32_t len = pl > skip ? pl - skip : 0;
            EXPECT(j.status == (len > 4080 ? -ERANGE : 0));
            EXPECT(j.status || (j.offset == (uint64_t(1) << 40) + 15 + skip && j.len == len && !j.uplink &&
                                j.fcnt == 0xFFFF));
            EXPECT(lw_crypt_job_tx(*t, 9, skip).status == -ENOKEY);
            t->fopts_len = 16;
            EXPECT(lw_crypt_job_tx(*t, 9, skip).status == -EINVAL);
            t->fopts_len = 0, t->mtype = 8;
            EXPECT(lw_crypt_job_tx(*t, 10, skip).status == -EINVAL);
        }
    for (uint32_t skip = 0; skip < 2; ++skip) {
        std::unique_ptr<lphy_ragged_desc> d(new lphy_ragged_desc{});
        std::unique_ptr<lphy_lorawan_frame> r(new lphy_lorawan_frame{});
        d->samples = (2 * 40 + 2) * 128, d->sym_offset = 2001;  // a row of 40 bytes at byte 1000
        r->status = 20, r->payload_offset = 16, r->payload_len = 20, r->devaddr = 5, r->fcnt = 6, r->mhdr = 0x40;
        LwCryptJob j = lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip);
        EXPECT(j.status == 0 && j.offset == 1016 + skip && j.len == 20 - skip && j.uplink && j.key == 1);
        r->mhdr = 0x60;
        EXPECT(!lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).uplink);
        r->payload_len = 21;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -EINVAL);
        r->payload_len = 0xFFFFFFFFu;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -EINVAL);
        r->payload_len = 0, r->payload_offset = 7;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -EINVAL);
        r->payload_offset = 36;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == 0);
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).len == 0);
        EXPECT(lw_crypt_job_rx(*d, *r, 2, 128, 1, 2, skip).status == -ENOKEY);
        EXPECT(lw_crypt_job_rx(*d, *r, kLwNoKey, 128, 1, uint64_t(1) << 40, skip).status == -ENOKEY);
        r->status = -EINVAL;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -EINVAL);
        r->status = -ENOKEY;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -ENOKEY);
        d->samples = uint64_t(1) << 31;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -ERANGE);
        // a row long enough for a range over the limit
        d->samples = (2 * 5000 + 2) * 128;
        r->status = 4081 + (int32_t)skip, r->payload_offset = 8, r->payload_len = 4081 + skip;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == -ERANGE);
        r->payload_len = 4080 + skip;
        EXPECT(lw_crypt_job_rx(*d, *r, 1, 128, 1, 2, skip).status == 0);
    }
    std::printf("lorawan_crypt_check: ok\n");
    return 0;
}
#endif
