"""The ring arithmetic of DeviceReplayBuffer (head, count, start, ex // aug, ex % aug, the padded record stride) without a
GPU: the buffer only needs an object with n, record_bytes and examples_gather(...).  Here that object is numpy: it reads the
ring through the pointers it is handed, checks every index against the ring's bounds and applies the independent reference
(tests/examples_ref.py).  The model is the reference's own buffer: a collections.deque(maxlen=capacity in positions)."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from tests import examples_ref as ref

from alphazero_piskvorky_amd.device_replay import DeviceReplayBuffer


class NumpyEngine:
    """Stand-in for Engine: az_examples_gather on host memory."""

    def __init__(self, n):
        self.n = n
        self.record_bytes = ref.record_bytes(n)
        self.ring_records = None          # set by the test: how many records the ring holds
        self.max_sym = 7
        self.calls = 0

    def examples_gather(self, packed_ptr, idx_ptr, sym_ptr, count, reference_pi, states_ptr, pis_ptr, z_ptr):
        self.calls += 1
        if count == 0:
            return
        n, nn, rb = self.n, self.n * self.n, self.record_bytes
        assert packed_ptr and idx_ptr and sym_ptr and states_ptr and pis_ptr and z_ptr
        idx = np.ctypeslib.as_array((C.c_int64 * count).from_address(idx_ptr)).copy()
        sym = np.ctypeslib.as_array((C.c_int32 * count).from_address(sym_ptr)).copy()
        assert idx.min() >= 0 and idx.max() < self.ring_records, "record index outside the ring"
        assert sym.min() >= 0 and sym.max() <= self.max_sym
        ring = np.ctypeslib.as_array((C.c_uint8 * (self.ring_records * rb)).from_address(packed_ptr))
        st, pi, z = ref.expected_gather(ref.unpack(ring, n), n, idx, sym, reference_pi)
        np.ctypeslib.as_array((C.c_float * (count * 4 * nn)).from_address(states_ptr))[:] = st.reshape(-1)
        np.ctypeslib.as_array((C.c_float * (count * nn)).from_address(pis_ptr))[:] = pi.reshape(-1)
        np.ctypeslib.as_array((C.c_float * count).from_address(z_ptr))[:] = z


@pytest.mark.parametrize("aug", [1, 4, 8])
@pytest.mark.parametrize("n", [5, 14])              # 168 B unpadded | 852 -> 856 B padded
@pytest.mark.parametrize("capacity", [40, 41, 7, None])
def test_ring_follows_a_deque_of_positions(n, aug, capacity):
    capacity = aug if capacity is None else capacity
    rs = np.random.RandomState(1000 * n + 10 * aug + capacity)
    eng = NumpyEngine(n)
    buf = DeviceReplayBuffer(eng, capacity=capacity, aug=aug, device="cpu", seed=int(rs.randint(1 << 30)))
    cap = max(1, capacity // aug)
    assert buf.cap == cap and buf.ring.numel() == cap * ref.record_bytes(n)
    eng.ring_records, eng.max_sym = cap, aug - 1
    model = collections.deque(maxlen=cap)
    pool = ref.random_records(rs, n, 0)
    # an empty ring: nothing to sample, nothing to export
    ref.check_ring(buf, model, pool, n, aug)
    for step in range(200):
        op = rs.randint(4)
        if op < 2:
            R = int(rs.choice([0, 1, 2, 3, cap - 1, cap, cap + 1, 2 * cap + 3])) if rs.randint(3) == 0 else int(rs.randint(0, cap + 2))
            R = max(R, 0)
            new = ref.random_records(rs, n, R)
            first = len(pool["z"])
            pool = {k: np.concatenate([pool[k], new[k]]) for k in ref.FIELDS}
            # the padding bytes carry junk: nothing may depend on them
            buf.extend_packed(torch.from_numpy(ref.pack(new, n, fill=0xA5)), R)
            model.extend(range(first, first + R))
            assert len(buf) == len(model) * aug
        elif op == 2:
            ref.check_ring(buf, model, pool, n, aug)
        else:
            ref.check_ring(buf, model, pool, n, aug, sample=int(rs.randint(0, cap * aug + 1)))
    ref.check_ring(buf, model, pool, n, aug)
    assert eng.calls > 0


def test_reference_helpers_agree_with_themselves():
    """pack / unpack are inverses at every size (1 to 4 plane words, padded and unpadded strides), and the symmetry rule agrees
    with the C index map of the kernels restated in Python for every n and k."""
    rs = np.random.RandomState(7)
    for n in range(3, 16):
        rec = ref.random_records(rs, n, 9)
        rb = ref.record_bytes(n)
        assert rb % 8 == 0 and rb - (64 + 4 * n * n + 4) == (0 if n % 2 else 4)
        packed = ref.pack(rec, n, fill=0xFF)
        assert packed.size == 9 * rb and not ref.same(ref.unpack(packed, n), rec)
        x = np.arange(n * n, dtype=np.float32).reshape(1, n, n)
        for k in range(8):
            i, j = np.divmod(np.arange(n * n), n)
            si, sj = [(i, j), (j, n - 1 - i), (n - 1 - i, n - 1 - j), (n - 1 - j, i)][k & 3]
            if k >= 4:
                sj = n - 1 - sj
            assert np.array_equal(ref._sym(x, k).reshape(-1), (si * n + sj).astype(np.float32))
