"""Tensors past 2 GiB and 4 GiB on the device without large host arrays (tests/test_gpu_large.py, tests/test_large_plan.py).

* Operands are filled ON THE DEVICE by mi_op_fill_uniform (the splitmix64 counter stream of tests/synth.py; bf16 operands through
  mi_op_convert), so any element is rebuilt on the host from its flat index alone (`regen`): no operand is ever uploaded whole.
* Only slabs come back: whole images, copied from `pointer + byte offset` (`Arena.read`).  No host array here exceeds HOST_LIMIT bytes.
* The images of a case (`boundary_images`): 0, N - 1, the image n* that holds the element at byte offset 2^31 (and 2^32 where the tensor
  reaches it) with both neighbours, and two seeded ones.  A case that picks its own N takes it so that at least three whole images lie
  past the boundary (`need_past`).  Every channel of those images is checked: convref.slab_channels restricted to them selects a subset.
* References and bounds are convref's / ewref's float64 ones, unchanged (64 * 2^-24 * A; bf16 outputs between the RNE roundings).
* Reductions over the whole batch (weight gradients, BN statistics, BN' sums) take the SPARSE form: both operands are zeroed on the
  device, real data is uploaded into the slab images only, and the exact reference is the reduction over those images
  (`sparse_stats_ref`, `sparse_bn_stats`: convref.bn_stats_ref / ewref.stats_ref with the zero images taken analytically).  A kernel that
  wraps an offset (and so reads an image twice or not at all) or drops the high images disagrees.
* `Arena` counts the bytes of a case's own tensors (`peak`); an allocation that fails is an assertion, never a skip.
"""
import ctypes

import numpy as np

import convref as R
import synth

F32, BF16 = 0, 1
ITEM = {F32: 4, BF16: 2}
B31, B32 = 1 << 31, 1 << 32
HOST_LIMIT = 1 << 30
C_FACTOR, U24 = R.C_FACTOR, R.U24


# ---------------------------------------------------------------------------------------------------------------------------
# host side: any element from its flat index
def regen(seed, lo, hi, start, count, dt=F32):
    """elements [start, start + count) of a tensor mi_op_fill_uniform(seed, lo, hi) filled (dt = BF16: then rounded by mi_op_convert), as
    float32.  lo and hi are float32 numbers (the kernel widens them to double: tests/synth.py's arithmetic)"""
    assert count * 4 <= HOST_LIMIT, "a host array of %d bytes" % (count * 4)
    a = synth.uniform(seed, int(count), float(np.float32(lo)), float(np.float32(hi)), offset=int(start))
    return R.bf16_round32(a) if dt == BF16 else a


def regen_images(seed, lo, hi, images, E, dt=F32):
    """[len(images), E]: the images (E elements each) of a filled tensor"""
    return np.stack([regen(seed, lo, hi, n * E, E, dt) for n in images])


def boundary_images(N, E, itemsize, seed=0, need_past=3):
    """the images of a case whose tensor has N images of E elements of `itemsize` bytes (module docstring).  need_past: how many whole images
    must lie past the image that holds byte offset 2^31 (0: N is the planner's answer, not the case's choice)"""
    total = N * E * itemsize
    s = {0, N - 1}
    for b in (B31, B32):
        if total > b:
            n = b // (E * itemsize)                # the image that holds the element at byte offset b
            if b == B31:
                assert N - 1 - n >= need_past, "N = %d leaves %d whole images past byte 2^31 (image %d)" % (N, N - 1 - n, n)
            s.update((n - 1, n, n + 1))
    rng = np.random.RandomState(3000 + seed)
    s.update(int(i) for i in rng.randint(0, N, 2))
    return sorted(i for i in s if 0 <= i < N)


def crosses(N, E, itemsize, boundary=B31):
    return N * E * itemsize > boundary


def smallest_crossing_n(E, itemsize, boundary=B31, spare=3):
    """the smallest N whose tensor holds `spare` whole images past the image with the element at byte offset `boundary`"""
    return boundary // (E * itemsize) + spare + 1


# ---------------------------------------------------------------------------------------------------------------------------
# the sparse form of the whole-batch reductions
def sparse_stats_ref(ref, A, M):
    """convref.bn_stats_ref(ref_all, A_all) where ref_all / A_all are ref / A ([n, c, h, w], the slab images) and exact zeros in every other
    image of a batch of M samples per channel: float64 mean, biased variance and their bounds"""
    ax = (0, 2, 3)
    Ms = ref.shape[0] * ref.shape[2] * ref.shape[3]
    assert M >= Ms
    mu = ref.sum(ax) / M
    d = ref - mu[None, :, None, None]
    var = ((d * d).sum(ax) + (M - Ms) * mu * mu) / M
    bm = C_FACTOR * U24 * (np.abs(ref) + A).sum(ax) / M
    bv = C_FACTOR * U24 * (ref * ref + 2 * np.abs(d) * A).sum(ax) / M
    return mu, var, bm, bv


def sparse_bn_stats(x, M):
    """ewref.stats_ref(x_all) with x_all = x in the slab images and zero elsewhere (M samples per channel)"""
    x64 = x.astype(np.float64)
    ax = (0, 2, 3)
    Ms = x.shape[0] * x.shape[2] * x.shape[3]
    mu = x64.sum(ax) / M
    d = x64 - mu[None, :, None, None]
    var = ((d * d).sum(ax) + (M - Ms) * mu * mu) / M
    return mu, var, C_FACTOR * U24 * np.abs(x64).sum(ax) / M, C_FACTOR * U24 * (x64 * x64).sum(ax) / M


def stats_distance(gm, gv, stats):
    """channels of (gm, gv) outside the bounds of `stats` = (mu, var, bm, bv), and the worst distance in 2^-24 (bound scale) units"""
    mu, var, bm, bv = stats
    em, ev = np.abs(np.asarray(gm, np.float64) - mu), np.abs(np.asarray(gv, np.float64) - var)
    bad = int(np.count_nonzero(~(em <= bm))) + int(np.count_nonzero(~(ev <= bv)))
    return bad, float(max(np.max(em / bm), np.max(ev / bv))) * C_FACTOR


# ---------------------------------------------------------------------------------------------------------------------------
# device side
def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32)


class Arena:
    """the device tensors of one case: raw pointers from mi_malloc, the live and the peak byte count"""

    def __init__(self, L):
        self.L, self.live, self.now, self.peak = L, {}, 0, 0

    def alloc(self, count, dt=F32):
        nbytes = int(count) * ITEM[dt]
        p = self.L.mi_malloc(nbytes)
        assert p, "mi_malloc(%d bytes) failed with %d bytes live: %s" % (nbytes, self.now, self.L.mi_last_error().decode())
        self.live[p] = nbytes
        self.now += nbytes
        self.peak = max(self.peak, self.now)
        return p

    def free(self, p):
        self.now -= self.live.pop(p)
        self.L.mi_free(p)

    def close(self):
        for p in list(self.live):
            self.free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _ok(self, rc, what):
        assert rc == 0, "%s failed (%d): %s" % (what, rc, self.L.mi_last_error().decode())

    # ---- whole tensors, on the device only
    def fill(self, p, count, seed, lo, hi, dt=F32):
        """p[0 : count] = the stream `regen` restates (bf16: filled as fp32 in scratch, rounded by mi_op_convert)"""
        if dt == F32:
            return self._ok(self.L.mi_op_fill_uniform(p, count, seed, lo, hi), "mi_op_fill_uniform")
        tmp = self.alloc(count, F32)
        self._ok(self.L.mi_op_fill_uniform(tmp, count, seed, lo, hi), "mi_op_fill_uniform")
        self._ok(self.L.mi_op_convert(tmp, F32, p, BF16, count), "mi_op_convert")
        self.free(tmp)

    def zero(self, p, count, dt=F32):
        """exact zeros (mi_op_fill_uniform with lo = hi = 0; two bf16 zeros are one fp32 zero)"""
        assert dt == F32 or count % 2 == 0
        self._ok(self.L.mi_op_fill_uniform(p, count if dt == F32 else count // 2, 0, 0.0, 0.0), "mi_op_fill_uniform")

    def poison(self, p, count, dt=F32):
        """NaN in every element (lo = hi = NaN): an element the kernel leaves out is out of every bound"""
        self.fill(p, count, 0, float("nan"), float("nan"), dt)

    def new_filled(self, count, seed, lo, hi, dt=F32):
        p = self.alloc(count, dt)
        self.fill(p, count, seed, lo, hi, dt)
        return p

    def new_zero(self, count, dt=F32):
        p = self.alloc(count, dt)
        self.zero(p, count, dt)
        return p

    def new_poisoned(self, count, dt=F32):
        p = self.alloc(count, dt)
        self.poison(p, count, dt)
        return p

    # ---- slabs
    def read(self, p, start, count, dt=F32):
        """elements [start, start + count) of the tensor at p, as float32 (int32 for dt = "i32")"""
        item = 4 if dt == "i32" else ITEM[dt]
        assert count * item <= HOST_LIMIT and (start + count) * item <= self.live[p]
        out = np.empty(count, {F32: np.float32, BF16: np.uint16, "i32": np.int32}[dt])
        self.L.mi_copy_to_host(out.ctypes.data, p + start * item, count * item)
        return _bf16_to_f32(out) if dt == BF16 else out

    def read_images(self, p, images, E, dt=F32):
        return np.stack([self.read(p, n * E, E, dt) for n in images])

    def write(self, p, start, arr, dt=F32):
        """elements [start, ...) of the tensor at p = arr (float32; bf16: uploaded to scratch and rounded by mi_op_convert)"""
        arr = np.ascontiguousarray(arr, np.float32).ravel()
        assert (start + arr.size) * ITEM[dt] <= self.live[p]
        if dt == F32:
            self.L.mi_copy_to_device(p + start * 4, arr.ctypes.data, arr.nbytes)
            return
        tmp = self.alloc(arr.size, F32)
        self.L.mi_copy_to_device(tmp, arr.ctypes.data, arr.nbytes)
        self._ok(self.L.mi_op_convert(tmp, F32, p + start * 2, BF16, arr.size), "mi_op_convert")
        self.free(tmp)

    def write_images(self, p, images, E, arr, dt=F32):
        for i, n in enumerate(images):
            self.write(p, n * E, arr[i], dt)

    def upload(self, arr, dtype=np.float32):
        """a small host array (weights, per-channel vectors, labels) as a device tensor of its own"""
        arr = np.ascontiguousarray(arr, dtype)
        p = self.L.mi_malloc(max(arr.nbytes, 4))
        assert p, "mi_malloc(%d bytes) failed: %s" % (arr.nbytes, self.L.mi_last_error().decode())
        self.live[p] = arr.nbytes
        self.now += arr.nbytes
        self.peak = max(self.peak, self.now)
        self.L.mi_copy_to_device(p, arr.ctypes.data, arr.nbytes)
        return p

    def download(self, p, count, dtype=np.float32):
        out = np.empty(count, dtype)
        self.L.mi_copy_to_host(out.ctypes.data, p, out.nbytes)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# which kernel ran, and the refusal half of the contract
def launched(L):
    buf = ctypes.create_string_buffer(96 * 100)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1]
    assert n == len(names), "the ring holds %d names, %d were returned" % (n, len(names))
    return names


def assert_launched(L, prefixes, what):
    """every prefix names a launch since the last mi_debug_trace_clear (RESNET_MI_TRACE=1: tests/conftest.py)"""
    names = launched(L)
    for pre in prefixes:
        assert any(n.startswith(pre) for n in names), "%s: no launch named %s*; launched %s" % (what, pre, names)
    return names


def assert_refused(L, rc, what):
    """the refusal: a non-zero return, mi_last_error names the size limit, no kernel was launched.  Clears the error"""
    err = L.mi_last_error().decode()
    names = launched(L)
    L.mi_clear_error()
    assert rc != 0, "%s: expected a refusal, the call returned 0" % what
    assert "size limit" in err, "%s refused (%d) without naming the size limit: %r" % (what, rc, err)
    assert not names, "%s refused (%d) but launched %s" % (what, rc, names)
    return err
