"""Independent model of the Poseidon252 Merkle channel, in plain Python integers, written from the public Starknet Poseidon
definition and the reference's TypeScript (vcs/poseidon252_merkle.ts, channel/poseidon.ts, backend/cpu/grind.ts).  It shares no
code with tstwo_amd/poseidon.py; the tests compare the library's host classes and kernels with it.

Field p = 2^251 + 17 2^192 + 1.  Hades: width 3, rounds 0-3 and 87-90 full, 4-86 partial; a round adds ARK[r], applies x^3
(all three elements, or s[2] only), and multiplies by [[3,1,1],[1,-1,1],[1,1,-2]].
"""
from __future__ import annotations

import hashlib

P = 2**251 + 17 * 2**192 + 1
M31_P = 2**31 - 1
ARK = [[int.from_bytes(hashlib.sha256(f"Hades{3 * i + j}".encode()).digest(), "big") % P for j in range(3)] for i in range(91)]


def hades(state):
    a, b, c = state
    for r in range(91):
        a, b, c = (a + ARK[r][0]) % P, (b + ARK[r][1]) % P, (c + ARK[r][2]) % P
        if r < 4 or r >= 87:
            a, b = pow(a, 3, P), pow(b, 3, P)
        c = pow(c, 3, P)
        a, b, c = (3 * a + b + c) % P, (a - b + c) % P, (a + b - 2 * c) % P
    return [a, b, c]


def hash_many(values):
    v = [x % P for x in values] + [1]
    if len(v) % 2:
        v.append(0)
    s = [0, 0, 0]
    for k in range(0, len(v), 2):
        s = hades([(s[0] + v[k]) % P, (s[1] + v[k + 1]) % P, s[2]])
    return s[0]


def hash2(x, y):
    """poseidonHash(x, y): one permutation of [x, y, 2]."""
    return hades([x % P, y % P, 2])[0]


def pack8(vals):
    """8 M31 values into one element, the first most significant (31 bits each)."""
    out = 0
    for v in vals:
        out = (out << 31) | int(v)
    return out


def hash_node(children, cols):
    items = list(children) if children is not None else []
    cols = [int(c) for c in cols]
    if len(cols) % 8:
        cols += [0] * (8 - len(cols) % 8)
    items += [pack8(cols[i:i + 8]) for i in range(0, len(cols), 8)]
    return hash_many(items)


def commit(columns):
    """Whole tree over columns (lists of ints, power-of-two lengths, mixed sizes): layers[k] = 2^k node values, layers[0] = [root]."""
    logs = [len(c).bit_length() - 1 for c in columns]
    max_log = max(logs) if columns else 0
    layers = {}
    prev = None
    for lg in range(max_log, -1, -1):
        cs = [c for c, l in zip(columns, logs) if l == lg]
        cur = [hash_node((prev[2 * i], prev[2 * i + 1]) if prev is not None else None, [c[i] for c in cs]) for i in range(1 << lg)]
        layers[lg] = cur
        prev = cur
    return [layers[k] for k in range(max_log + 1)]


def decommit(layers, columns, queries_per_log):
    """The reference walk (vcs/prover.ts:32-109) on the model tree: (queried values, hash witness, column witness)."""
    logs = [len(c).bit_length() - 1 for c in columns]
    max_log = len(layers) - 1
    queried, hashes, colwit = [], [], []
    last = []
    for lg in range(max_log, -1, -1):
        cs = [c for c, l in zip(columns, logs) if l == lg]
        direct = list(queries_per_log.get(lg, []))
        nodes = sorted(set([q // 2 for q in last] + direct))
        for node in nodes:
            if lg < max_log:
                for k in (2 * node, 2 * node + 1):
                    if k not in last:
                        hashes.append(layers[lg + 1][k])
            vals = [c[node] for c in cs]
            if node in direct:
                queried += vals
            else:
                colwit += vals
        last = nodes
    return queried, hashes, colwit


def to_words(x):
    """8 little-endian u32 limbs."""
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def from_words(w):
    return sum(int(v) << (32 * k) for k, v in enumerate(w))


def trailing_zeros(digest):
    """First 16 bytes of the big-endian encoding read as a little-endian u128."""
    v = int.from_bytes(digest.to_bytes(32, "big")[:16], "little")
    return 128 if v == 0 else (v & -v).bit_length() - 1


class Channel:
    """Poseidon252Channel (channel/poseidon.ts:122-360)."""

    def __init__(self):
        self.digest, self.n_challenges, self.n_sent = 0, 0, 0

    def clone(self):
        c = Channel()
        c.digest, c.n_challenges, c.n_sent = self.digest, self.n_challenges, self.n_sent
        return c

    def _update(self, d):
        self.digest, self.n_challenges, self.n_sent = d, self.n_challenges + 1, 0

    def mix_u32s(self, data):
        data = list(data) + [0] * (6 - (len(data) + 6) % 7)
        felts = []
        for i in range(0, len(data), 7):
            acc = 0
            for w in data[i:i + 7]:
                acc = (acc * 2**32 + w) % P
            felts.append(acc)
        self._update(hash_many([self.digest] + felts))

    def mix_u64(self, n):
        self.mix_u32s([0, 0, 0, 0, 0, n >> 32, n & 0xFFFFFFFF])

    def mix_felts(self, felts):
        """felts: QM31 values as 4-tuples of M31 ints."""
        res = [self.digest]
        for i in range(0, len(felts), 2):
            acc = 0
            for f in felts[i:i + 2]:
                for m in f:
                    acc = (acc * 2**31 + m) % P
            res.append(acc)
        self._update(hash_many(res))

    def mix_root(self, root):
        self._update(hash_many([self.digest, root]))

    def _draw252(self):
        r = hash2(self.digest, self.n_sent)
        self.n_sent += 1
        return r

    def draw_base_felts(self):
        cur = self._draw252()
        out = []
        for _ in range(8):
            out.append((cur % 2**31) % M31_P)
            cur //= 2**31
        return out

    def draw_felt(self):
        return tuple(self.draw_base_felts()[:4])

    def draw_felts(self, n):
        out, buf = [], []
        while len(out) < n:
            if len(buf) < 4:
                buf += self.draw_base_felts()
            out.append(tuple(buf[:4]))
            del buf[:4]
        return out

    def draw_random_bytes(self):
        cur = self._draw252()
        return bytes((cur >> (8 * i)) & 0xFF for i in range(31))

    def trailing_zeros(self):
        return trailing_zeros(self.digest)


def grind(digest, pow_bits, start=0):
    """The sequential reference loop from `start`: the first nonce whose mix_u64 gives >= pow_bits trailing zeros."""
    n = start
    while True:
        if trailing_zeros(hash_many([digest, n])) >= pow_bits:
            return n
        n += 1
