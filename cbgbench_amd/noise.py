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

Training and validation take the same mode (``model(batch, noise=CounterNoise(...))`` in training and in eval mode, ``train_cli --noise
counter``).  The key of a graph is ``stream_keys(seed, example index, visit)``: the example's index in its dataset -- a global identity --
stands where the pocket index stands, the training iteration (the same number on every rank) where the sample index stands
(``training_noise``); validation uses visit 0 under the purpose base ``PURPOSE_STRIDE`` (``validation_noise``), so it shares no address
with training.  The time of a graph is ``(uint64(w0) * n_t) >> 32`` with ``w0`` = word 0 at counter (0, 0, base + TRAIN_TIME, 0)
(``train_times``; n_t = T for TargetDiff and DiffBP, T + 1 for DiffSBDD); the per-atom draws (purposes TRAIN_*) use the graph's integer
time as their step word, in training and in eval mode.  What this gives up: every time keeps the symmetric sampler's marginal (uniform
on [0, T)), but the antithetic pairing t, T - 1 - t inside a batch is a function of batch position and is not kept; TargetDiff's
``time_sampler: uniform`` is refused rather than silently replaced.  What it does not separate: two evaluation times of one validation
call that coincide after truncation to an integer (tiny T) draw at the same addresses, hence get the same noise.  What it buys: the noised
inputs of an example at an iteration are the same for every world size, batch size and batch position, a validation loss is a function of
the weights, and a resumed run sees the noise the uninterrupted run saw.  (The gradients keep their fp32 atomics: the inputs of a step
are reproducible, not the step.)

The protein-coordinate augmentation of a training visit (the config's ``add_pos_noise``, applied by ``train_cli.apply_plan`` before the
model call; ``cbgx_train_transform_rng``) has its own purpose, TRAIN_PROTEIN_NORMAL: counter = (the protein atom's index inside its pocket,
step 0, base + TRAIN_PROTEIN_NORMAL, block 0), components 0..2, under the graph's training / validation key above -- it does not depend on
the graph's time.  Precondition: the protein atoms of an example keep their order.  ``protein_draw_model`` / ``protein_addresses`` are its
numpy model; ``train_addresses`` / ``validation_addresses`` list the draws of the model call only, as before.

Which decomposition of its ligand a visit trains on (the config's ``choose_ctx_gen``; ``cbgx_train_transform_choose_rng``, in the same
launch as the protein noise and the centring) is drawn at the purpose TRAIN_CHOOSE_CTX: k = ``scale_word``(word 0 of the call at counter
(0, 0, base + TRAIN_CHOOSE_CTX, 0), K) under the graph's key -- the time's formula at an address of its own.  ``choose_model`` /
``choose_addresses`` are its numpy model.

The numpy functions below restate the generator from its definition (Salmon et al., SC'11); tests compare the header (built with a
host compiler) and the kernels against them: words and uniforms bit for bit, normals within the rounding of the device's
logf / sqrtf / sincosf.
"""
import numpy as np
import torch

from . import _native

# purposes (csrc/rng.h ``Purpose``, include/cbgx.h CBGX_NOISE_*)
POS_NORMAL, TYPE_UNIFORM, MASK_UNIFORM, TYPE_NORMAL, INIT_POS, INIT_TYPE, FINAL_POS = range(7)
TRAIN_TIME, TRAIN_POS_NORMAL, TRAIN_TYPE_UNIFORM, TRAIN_MASK_UNIFORM, TRAIN_TYPE_NORMAL, TRAIN_PROTEIN_NORMAL = range(7, 13)
TRAIN_CHOOSE_CTX = 13       # the decomposition choice of a visit (not a per-atom draw; PURPOSE_NAMES lists those)
PURPOSE_STRIDE = 16
PURPOSE_NAMES = ("pos_normal", "type_uniform", "mask_uniform", "type_normal", "init_pos", "init_type", "final_pos",
                 "train_time", "train_pos_normal", "train_type_uniform", "train_mask_uniform", "train_type_normal",
                 "train_protein_normal")
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
    call with counter (a - lig_ptr[graph], step, purpose, col // 4) under the graph's key.  ``step``: one integer, or one per atom as
    an [n_lig, 1] array (training: the time of the atom's graph)"""
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


def scale_word(w, n):
    """``rng::scale_word``: (uint64(w) * n) >> 32 in [0, n) -- 0xFFFFFFFF gives n - 1, never n"""
    return ((np.asarray(w, dtype=np.uint64) & _MASK) * np.uint64(n)) >> np.uint64(32)


def train_times(keys, n_t, purpose_base=0):
    """``rng::train_time``: [B] int64 times in [0, n_t) of the graphs with stream keys ``keys``"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((keys.size, 4), dtype=np.uint64)
    ctr[:, 2] = purpose_base + TRAIN_TIME
    key = np.stack([keys & _MASK, keys >> np.uint64(32)], -1)
    return scale_word(philox4x32_10(ctr, key)[:, 0], n_t).astype(np.int64)


def train_draw_model(keys, lig_ptr, n_t, purpose_base=0, cols_b=0, purpose_b=TRAIN_TYPE_UNIFORM, uniform_b=True, t_in=None):
    """numpy model of ``cbgx_train_noise_draw``: (t [B] int64, a [n_lig, 3] float64 normals, b [n_lig, cols_b] fp32 uniforms (bit-exact)
    or float64 normals, None when ``cols_b`` is 0) -- ``fill_model`` with the time of the atom's graph as the step"""
    lig_ptr = np.asarray(lig_ptr, dtype=np.int64)
    t = train_times(keys, n_t, purpose_base) if t_in is None else np.asarray(t_in, dtype=np.int64).reshape(-1).copy()
    step = np.repeat(t, np.diff(lig_ptr))[:, None]
    a = fill_model(keys, lig_ptr, step, purpose_base + TRAIN_POS_NORMAL, 3, False)
    b = fill_model(keys, lig_ptr, step, purpose_base + purpose_b, cols_b, uniform_b) if cols_b else None
    return t, a, b


def protein_draw_model(keys, rec_ptr, purpose_base=0):
    """numpy model of the normals ``cbgx_train_transform_rng`` draws: [n_rec, 3] float64, atom ``a`` of graph ``g`` at counter
    (a - rec_ptr[g], 0, purpose_base + TRAIN_PROTEIN_NORMAL, 0) under ``keys[g]`` -- ``fill_model`` on the protein CSR at step 0"""
    return fill_model(keys, rec_ptr, 0, purpose_base + TRAIN_PROTEIN_NORMAL, 3, False)


def protein_addresses(keys, rec_ptr, purpose_base=0):
    """the (key, atom, step, purpose, block) addresses of ``protein_draw_model``: [n_rec, 5] uint64, one row (one Philox call) per atom"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.diff(np.asarray(rec_ptr, dtype=np.int64))
    rows = [(keys[g], a, 0, purpose_base + TRAIN_PROTEIN_NORMAL, 0) for g, n in enumerate(counts) for a in range(int(n))]
    return np.array(rows, dtype=np.uint64).reshape(-1, 5)


def choose_model(keys, K, purpose_base=0):
    """numpy model of the choice ``cbgx_train_transform_choose_rng`` draws: [B] int64, graph ``g`` with ``K[g]`` decompositions (one
    integer: the same for all) gets ``scale_word``(word 0 at counter (0, 0, purpose_base + TRAIN_CHOOSE_CTX, 0) under ``keys[g]``, K[g])
    in [0, K[g]); -1 where K[g] is 0"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    K = np.broadcast_to(np.asarray(K, dtype=np.int64), keys.shape)
    if K.size and K.min() < 0:
        raise ValueError("choose_model: K must be >= 0")
    ctr = np.zeros((keys.size, 4), dtype=np.uint64)
    ctr[:, 2] = purpose_base + TRAIN_CHOOSE_CTX
    key = np.stack([keys & _MASK, keys >> np.uint64(32)], -1)
    w0 = philox4x32_10(ctr, key)[:, 0].astype(np.uint64)
    k = ((w0 * K.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return np.where(K > 0, k, -1)


def choose_addresses(keys, purpose_base=0):
    """the (key, atom, step, purpose, block) addresses of ``choose_model``: [B, 5] uint64, one row (one Philox call) per graph"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    return np.array([(k, 0, 0, purpose_base + TRAIN_CHOOSE_CTX, 0) for k in keys], dtype=np.uint64).reshape(-1, 5)


TRAIN_PURPOSE_B = {"targetdiff": TRAIN_TYPE_UNIFORM, "diffbp": TRAIN_MASK_UNIFORM, "diffsbdd": TRAIN_TYPE_NORMAL}


def eval_times(model_type, T, eval_interval):
    """the integer times of one eval-mode ``forward`` (what the model classes truncate their ``linspace`` to)"""
    lin = np.linspace(1, T, eval_interval) if model_type == "diffsbdd" else np.linspace(0, T - 1, eval_interval)
    return [int(v) for v in lin]


def _call_addresses(model_type, keys, lig_ptr, t, C, purpose_base):
    counts = np.diff(np.asarray(lig_ptr, dtype=np.int64))
    blocks_b = 1 if model_type == "diffbp" else (C + 3) // 4
    rows = []
    for g, n in enumerate(counts):
        for a in range(int(n)):
            rows.append((keys[g], a, int(t[g]), purpose_base + TRAIN_POS_NORMAL, 0))
            rows += [(keys[g], a, int(t[g]), purpose_base + TRAIN_PURPOSE_B[model_type], b) for b in range(blocks_b)]
    return rows


def train_addresses(model_type, keys, lig_ptr, T, C, purpose_base=0, t_in=None):
    """every (key, atom, step, purpose, block) address ONE training call of ``model_type`` draws from, [n, 5] uint64, one row per
    Philox call: the time of every graph (not with ``t_in``: given times draw nothing) and the per-atom draws at that time"""
    keys = np.asarray(keys, dtype=np.uint64)
    n_t = T + 1 if model_type == "diffsbdd" else T
    rows = []
    if t_in is None:
        rows = [(k, 0, 0, purpose_base + TRAIN_TIME, 0) for k in keys]
        t_in = train_times(keys, n_t, purpose_base)
    rows += _call_addresses(model_type, keys, lig_ptr, t_in, C, purpose_base)
    return np.array(rows, dtype=np.uint64).reshape(-1, 5)


def validation_addresses(model_type, keys, lig_ptr, T, C, eval_interval, purpose_base=PURPOSE_STRIDE):
    """the addresses of ONE eval-mode call, evaluation time after evaluation time in call order (DiffSBDD: per time the draws at the
    time and the draws of its second network call at step 0) -- a list with one [n, 5] array per draw call, so that a test can tell the
    documented repetition (two evaluation times equal after truncation) from an overlap"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = []
    for tv in eval_times(model_type, T, eval_interval):
        out.append(np.array(_call_addresses(model_type, keys, lig_ptr, [tv] * keys.size, C, purpose_base), dtype=np.uint64).reshape(-1, 5))
        if model_type == "diffsbdd":
            out.append(np.array(_call_addresses(model_type, keys, lig_ptr, [0] * keys.size, C, purpose_base), dtype=np.uint64).reshape(-1, 5))
    return out


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
            host = torch.from_numpy(self.keys.view(np.int64).copy())
            if torch.device(device).type == "cuda":
                # from pinned memory, without waiting: a pageable copy would make the host wait for everything queued on the stream,
                # and a training step builds a new CounterNoise every iteration (measured: + 0.4 ... 1 ms per 32-graph step)
                self._dev[k] = host.pin_memory().to(device, non_blocking=True)
            else:
                self._dev[k] = host.to(device)
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


def ligand_csr(bl, B):
    """[B + 1] int32 offsets of the graphs' ligands in ligand arrays sorted by graph (``bl``: the graph of every ligand atom)"""
    return torch.cat([torch.zeros(1, dtype=torch.long, device=bl.device),
                      torch.bincount(bl, minlength=B).cumsum(0)]).to(torch.int32).contiguous()


def attach(st, noise, bl, B, lig_ptr=None, ordered=None):
    """put the operands of the counter mode into a sampling state: keys, the per-atom graph and the ligand CSR (int32).  ``lig_ptr`` /
    ``ordered``: that CSR and whether ``bl`` is sorted, from a caller that has them already (the state builder looks once and builds
    once); without them both are worked out here."""
    if noise is None:
        return st
    dev = bl.device
    if dev.type != "cuda":
        raise ValueError("counter noise is generated by the GPU kernels: the sampling state must live on the GPU")
    if noise.num_graphs != B:
        raise ValueError(f"noise has {noise.num_graphs} stream keys for a batch of {B} graphs")
    if not (bool((bl[1:] >= bl[:-1]).all()) if ordered is None else ordered):
        raise ValueError("counter noise needs the ligand atoms sorted by graph (an atom is addressed by its index inside its ligand)")
    st["noise"] = noise
    st["noise_keys"] = noise.device_keys(dev)
    st["noise_graph"] = bl.to(torch.int32).contiguous()
    st["noise_ptr"] = ligand_csr(bl, B) if lig_ptr is None else lig_ptr
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


# ---- training and validation -----------------------------------------------------------------------------------------------------
def training_noise(seed, example_index, iteration):
    """the ``noise=`` of the training call of iteration ``iteration`` on the examples ``example_index`` [B] (indices in the dataset)"""
    ex = np.asarray(example_index, dtype=np.int64).reshape(-1)
    return CounterNoise(seed, ex, np.full(ex.shape, int(iteration), dtype=np.int64), purpose_base=0)


def validation_noise(seed, example_index):
    """the ``noise=`` of a validation call on the examples ``example_index``: visit 0, purpose base PURPOSE_STRIDE"""
    ex = np.asarray(example_index, dtype=np.int64).reshape(-1)
    return CounterNoise(seed, ex, np.zeros(ex.shape, dtype=np.int64), purpose_base=PURPOSE_STRIDE)


def train_operands(noise, batch, B):
    """the operands of the counter mode of one ``get_loss`` call: (keys [B] int64 bits, lig_ptr [B+1] int32, noise) on the batch's device.
    A batch that carries ``ligand_ptr`` (``ComplexSet.collate(..., example_ids=True)``: built on the host from the ligand sizes, so the
    atoms are sorted by construction) spares the check and the prefix sum their launches and their host synchronisation."""
    bl = batch["ligand_element_batch"]
    if noise.num_graphs != B:
        raise ValueError(f"noise has {noise.num_graphs} stream keys for a batch of {B} graphs")
    ptr = batch.get("ligand_ptr", None)
    if ptr is None and not bool((bl[1:] >= bl[:-1]).all()):
        raise ValueError("counter noise needs the ligand atoms sorted by graph (an atom is addressed by its index inside its ligand)")
    dev = bl.device
    if dev.type != "cuda":
        raise ValueError("counter noise is generated by the GPU kernels: the batch must live on the GPU")
    if ptr is None:
        ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.bincount(bl, minlength=B).cumsum(0)]).to(torch.int32)
        if ptr.shape[0] != B + 1:
            raise ValueError(f"noise has {noise.num_graphs} stream keys for a batch of {ptr.shape[0] - 1} graphs")
    elif ptr.dtype != torch.int32 or ptr.shape[0] != B + 1 or ptr.device != dev:
        raise ValueError("ligand_ptr must be the [B + 1] int32 ligand CSR on the batch's device")
    return noise.device_keys(dev), ptr.contiguous(), noise


def train_draw(ops, n_lig, n_t, t_in=None, cols_b=0, purpose_b=TRAIN_TYPE_UNIFORM, uniform_b=True, positions=True):
    """``cbgx_train_noise_draw`` on the current stream: (t [B] int64 -- ``t_in``, or drawn --, a [n_lig, 3] normals or None,
    b [n_lig, cols_b] or None), both at the step t[graph]"""
    keys, ptr, noise = ops
    dev, B = keys.device, int(keys.shape[0])
    t_out = torch.empty(B, dtype=torch.int64, device=dev)
    a = torch.empty(n_lig, 3, dtype=torch.float32, device=dev) if positions else None
    b = torch.empty(n_lig, cols_b, dtype=torch.float32, device=dev) if cols_b else None
    if t_in is not None:
        t_in = t_in.to(device=dev, dtype=torch.int64).contiguous()
        if t_in.shape[0] != B:
            raise ValueError(f"t has {t_in.shape[0]} entries for a batch of {B} graphs")
    _native.check(_native.lib().cbgx_train_noise_draw(
        _native.ptr(keys), _native.ptr(ptr), B, int(n_lig), noise.purpose_base, int(n_t), _native.ptr(t_in), _native.ptr(t_out),
        _native.ptr(a), _native.ptr(b), int(cols_b), int(purpose_b), int(bool(uniform_b)), _native.current_stream(dev)),
        "cbgx_train_noise_draw")
    return t_out, a, b
