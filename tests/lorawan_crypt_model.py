"""The FRMPayload cipher of LoRaWAN 1.0.x 4.3.3 restated from the specification's
text, for tests/test_lorawan_crypt_cpu.py and tests/test_gpu_lorawan_crypt.py.
Nothing here is taken from the kernel: the block layout is the specification's,
and AES-128 is a checker's (tests/checkers.py: the oracle's, and the
reference's tiny-AES where it was built; the two must agree).

For a payload of len bytes, k = ceil(len / 16), and i = 1..k:
  A_i = 0x01 | 4 x 0x00 | Dir | DevAddr (4, little endian) | FCnt (4, little
        endian) | 0x00 | i          Dir = 0 uplink, 1 downlink
  S_i = aes128_encrypt(K, A_i),  S = S_1 | S_2 | .. | S_k
and the payload is XORed with the first len bytes of S."""
import numpy as np


def block_a(uplink, devaddr, fcnt, i) -> bytes:
    assert 1 <= i <= 255
    return (bytes([0x01, 0, 0, 0, 0, 0 if uplink else 1]) + int(devaddr).to_bytes(4, "little")
            + int(fcnt).to_bytes(4, "little") + bytes([0x00, i]))


class Cipher:
    """keystream() / crypt() on a list of AES-128 checkers that must agree."""

    def __init__(self, *aes):
        assert aes
        self.aes = aes

    def block_s(self, key, uplink, devaddr, fcnt, i) -> np.ndarray:
        a = block_a(uplink, devaddr, fcnt, i)
        s = [np.asarray(x.aes128(key, a), np.uint8) for x in self.aes]
        for t in s[1:]:
            assert np.array_equal(s[0], t), "the AES checkers disagree"
        return s[0]

    def keystream(self, key, uplink, devaddr, fcnt, n) -> np.ndarray:
        assert 0 <= n <= 255 * 16
        k = (n + 15) // 16
        if not k:
            return np.zeros(0, np.uint8)
        return np.concatenate([self.block_s(key, uplink, devaddr, fcnt, i) for i in range(1, k + 1)])[:n]

    def crypt(self, key, uplink, devaddr, fcnt, data) -> np.ndarray:
        d = np.frombuffer(bytes(data), np.uint8)
        return d ^ self.keystream(key, uplink, devaddr, fcnt, d.size)


def checkers_cipher() -> Cipher:
    """On the oracle's AES and, where the reference was built, on its too."""
    from checkers import Oracle, Reference, reference_available
    aes = [Oracle()]
    if reference_available():
        aes.append(Reference())
    return Cipher(*aes)
