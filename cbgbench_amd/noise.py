"""Counter-based noise of the samplers ("counter" noise mode): the host side and a numpy model of ``csrc/rng.h``.

In this mode every random number of a sampling run is a pure function of an address,

    Philox4x32-10(counter = (atom's index inside its ligand, step, purpose, block), key = the graph's 64-bit stream key)

evaluated on the device inside the kernel that consumes it (``cbgx_targetdiff_*_rng``) or by ``cbgx_noise_fill`` right in front of
it (DiffBP, DiffSBDD).  The stream key of a graph comes from (seed, pocket index, sample index) by one Philox call
(``stream_keys``).  The samples of graph (pocket p, sample s) at a seed are therefore the same whatever else is in the batch, in
whatever order, on however many ranks and streams, with or without a captured hipGraph.  The one precondition: the atoms of a
ligand keep their order (an atom is addressed by its index inside its ligand).

``CounterNoise(seed, pocket_index, sample_index)`` is what ``sample`` / ``sample_many`` / ``begin_sampling`` / ``denoise_step`` of
the three model classes take as ``noise=``; ``priors.build_sampling_batch(..., sample_streams=(seed, pocket_ids))`` puts one into
the batch it builds (key ``noise_keys``), with priors that have the same property.

The numpy functions below restate the generator from its definition (Salmon et al., SC'11); tests compare the header (built with a
host compiler) and the kernels against them: words and uniforms bit for bit, normals within the rounding of the device's
logf / sqrtf / sincosf.
"""
import numpy as np
import torch

from . import _native

# purposes (csrc/rng.h ``Purpose``, include/cbgx.h CBGX_NOISE_*)
POS_NORMAL, TYPE_UNIFORM, MASK_UNIFORM, TYPE_NORMAL, INIT_POS, INIT_TYPE, FINAL_POS = range(7)
PURPOSE_STRIDE = 16
PURPOSE_NAMES = ("pos_normal", "type_uniform", "mask_uniform", "type_normal", "init_pos", "init_type", "final_pos")
STREAM_KEY = (0x58474243, 0x53494F4E)

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """``counter`` [..., 4], ``key`` [..., 2] (anything that casts to uint32, broadcast against each other) -> words [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2           # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def stream_keys(seed, pocket_index, sample_index):
    """[B] uint64 stream keys of the graphs (pocket_index[g], sample_index[g]) at ``seed`` (``rng::stream_key``)."""
    p = np.asarray(pocket_index, dtype=np.int64).reshape(-1)
    s = np.asarray(sample_index, dtype=np.int64).reshape(-1)
    if p.shape != s.shape:
        raise ValueError(f"stream_keys: {p.shape[0]} pocket indices but {s.shape[0]} sample indices")
    if p.size and (min(p.min(), s.min()) < 0 or max(p.max(), s.max()) >= 1 << 32):
        raise ValueError("stream_keys: pocket and sample indices must be in [0, 2^32)")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.stack([np.full(p.shape, seed & 0xFFFFFFFF), np.full(p.shape, seed >> 32), p, s], -1)
    w = philox4x32_10(ctr, np.array(STREAM_KEY)).astype(np.uint64)
    return w[:, 0] | (w[:, 1] << np.uint64(32))


def words(keys, lig_ptr, step, purpose, cols):
    """the words behind ``cbgx_noise_fill``: [n_lig, cols] uint32, word of component ``col`` of atom ``a`` = output ``col % 4`` of the
    call with counter (a - lig_ptr[graph], step, purpose, col // 4) under the graph's key"""
    keys = np.asarray(keys, dtype=np.uint64)
    lig_ptr = np.asarray(lig_ptr, dtype=np.int64)
    counts = np.diff(lig_ptr)
    graph = np.repeat(np.arange(counts.size), counts)
    local = np.arange(int(lig_ptr[-1])) - lig_ptr[graph]
    nblk = (cols + 3) // 4
    ctr = np.empty((local.size, nblk, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = local[:, None], step, purpose, np.arange(nblk)[None, :]
    key = np.stack([keys[graph] & _MASK, keys[graph] >> np.uint64(32)], -1)[:, None, :]
    return philox4x32_10(ctr, key).reshape(local.size, nblk * 4)[:, :cols]


def uniforms(w):
    """(w >> 8) * 2^-24 in [0, 1), fp32 (exact)"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def normals(w, dtype=np.float64):
    """Box-Muller on the word pairs (0, 1), (2, 3), ... of the last axis (padded to even with a call's next word by the caller: pass the
    words of whole blocks): components (2 i, 2 i + 1) = r cos, r sin.  ``dtype`` float64: the exact value of the formula on the fp32
    inputs u_r = ((w_r >> 8) + 1) * 2^-24 and theta = fl32(fl32(2 pi) * u_a)."""
    w = np.asarray(w, dtype=np.uint32)
    if w.shape[-1] % 2:
        raise ValueError("normals: pass whole pairs of words")
    wr, wa = w[..., 0::2], w[..., 1::2]
    ur = ((wr >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    theta = (np.float32(6.283185307179586) * uniforms(wa)).astype(np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(ur))
    out = np.empty(w.shape, dtype=np.float64)
    out[..., 0::2], out[..., 1::2] = r * np.cos(theta), r * np.sin(theta)
    return out.astype(dtype)


def fill_model(keys, lig_ptr, step, purpose, cols, uniform):
    """numpy model of ``cbgx_noise_fill``: uniforms fp32 (bit-exact), normals float64"""
    w = words(keys, lig_ptr, step, purpose, 4 * ((cols + 3) // 4))
    return uniforms(w)[:, :cols] if uniform else normals(w)[:, :cols]


def run_addresses(model_type, keys, lig_ptr, T, C):
    """every (key, atom, step, purpose, block) address a sampling run of ``model_type`` over T steps draws from, as an [n, 5] uint64
    array (one row per Philox call) -- the model of the addressing that the host and the kernels follow"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.diff(np.asarray(lig_ptr, dtype=np.int64))
    nblk = (C + 3) // 4
    per_step = {"targetdiff": [(POS_NORMAL, 1), (TYPE_UNIFORM, nblk)],
                "diffbp": [(POS_NORMAL, 1), (MASK_UNIFORM, 1)],
                "diffsbdd": [(POS_NORMAL, 1), (TYPE_NORMAL, nblk)]}[model_type]
    once = [(INIT_POS, 1), (INIT_TYPE, nblk), (FINAL_POS, 1)] if model_type == "diffsbdd" else []
    rows = []
    for g, n in enumerate(counts):
        for a in range(int(n)):
            for purpose, blocks in once:
                rows += [(keys[g], a, 0, purpose, b) for b in range(blocks)]
            for t in range(T):
                for purpose, blocks in per_step:
                    rows += [(keys[g], a, t, purpose, b) for b in range(blocks)]
    return np.array(rows, dtype=np.uint64).reshape(-1, 5)


class CounterNoise:
    """The ``noise=`` argument that selects the counter mode: the stream keys of the B graphs of a batch, in batch order.
    ``pocket_index`` / ``sample_index`` [B]: which (pocket, sample) of the job graph g is -- a global identity, not a position."""

    def __init__(self, seed, pocket_index, sample_index, purpose_base=0):
        if purpose_base < 0 or purpose_base % PURPOSE_STRIDE:
            raise ValueError(f"purpose_base must be a non-negative multiple of {PURPOSE_STRIDE}")
        self.seed, self.purpose_base = int(seed), int(purpose_base)
        self.pocket_index = np.asarray(pocket_index, dtype=np.int64).reshape(-1).copy()
        self.sample_index = np.asarray(sample_index, dtype=np.int64).reshape(-1).copy()
        self.keys = stream_keys(seed, self.pocket_index, self.sample_index)
        self._dev = {}

    @property
    def num_graphs(self):
        return int(self.keys.shape[0])

    def device_keys(self, device):
        """[B] int64 tensor holding the uint64 keys' bits"""
        k = str(device)
        if k not in self._dev:
            self._dev[k] = torch.from_numpy(self.keys.view(np.int64).copy()).to(device)
        return self._dev[k]

    def __repr__(self):
        return f"CounterNoise(seed={self.seed}, graphs={self.num_graphs}, purpose_base={self.purpose_base})"


def resolve(noise, batch=None):
    """the CounterNoise of a call: the explicit argument, else the one the batch constructor left in the batch, else None"""
    if noise is None and batch is not None:
        noise = batch.get("noise_keys", None)
    if noise is not None and not isinstance(noise, CounterNoise):
        raise TypeError(f"noise= takes a CounterNoise (or None for the torch generator), not {type(noise).__name__}")
    return noise


def attach(st, noise, bl, B):
    """put the operands of the counter mode into a sampling state: keys, the per-atom graph and the ligand CSR (int32)"""
    if noise is None:
        return st
    dev = bl.device
    if dev.type != "cuda":
        raise ValueError("counter noise is generated by the GPU kernels: the sampling state must live on the GPU")
    if noise.num_graphs != B:
        raise ValueError(f"noise has {noise.num_graphs} stream keys for a batch of {B} graphs")
    if not bool((bl[1:] >= bl[:-1]).all()):
        raise ValueError("counter noise needs the ligand atoms sorted by graph (an atom is addressed by its index inside its ligand)")
    st["noise"] = noise
    st["noise_keys"] = noise.device_keys(dev)
    st["noise_graph"] = bl.to(torch.int32).contiguous()
    st["noise_ptr"] = torch.cat([torch.zeros(1, dtype=torch.long, device=dev),
                                 torch.bincount(bl, minlength=B).cumsum(0)]).to(torch.int32).contiguous()
    return st


def fill(st, purpose, step, cols, uniform, out=None, step_dev=None):
    """``cbgx_noise_fill`` on a state prepared by ``attach``: [n_lig, cols] draws of ``purpose`` at ``step`` on the current stream"""
    dev = st["noise_keys"].device
    n_lig = int(st["noise_graph"].shape[0])
    if out is None:
        out = torch.empty(n_lig, cols, dtype=torch.float32, device=dev)
    _native.check(_native.lib().cbgx_noise_fill(
        _native.ptr(st["noise_keys"]), _native.ptr(st["noise_ptr"]), int(st["noise_keys"].shape[0]), n_lig, int(cols), int(bool(uniform)),
        st["noise"].purpose_base + int(purpose), int(step), _native.ptr(step_dev), _native.ptr(out), _native.current_stream(dev)),
        "cbgx_noise_fill")
    return out
