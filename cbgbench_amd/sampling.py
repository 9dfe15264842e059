"""The sampling host path the three sampler classes (TargetDiff, DiffBP, DiffSBDD) share: everything around the network call of a
reverse-diffusion step that is not the class's own arithmetic.

* the sampling state (a plain dict; DESIGN.md 5, "The sampling state") is built in two parts, ``_plan_sampling`` and ``_finish_state`` --
  DiffSBDD draws its initial state between them;
* ``_run_denoiser`` is the one denoiser call of a step, ``_attach_noise`` / ``_adopt_noise`` put a ``CounterNoise`` into a state,
  ``_trajectory`` turns the device-resident slots into the returned dict;
* ``_sample_loop`` and ``sample_many`` drive a class through its hooks ``_many_begin`` / ``_many_step`` / ``_many_finish``.
"""
import os
import time

import torch
import torch.nn.functional as F

from . import _native
from . import noise as _noise
from .unitransformer import graph_ptr_from_batch

NUM_AA = 20          # len(aa_name_number), repo/utils/protein/constants.py:39

# the uint8 / int32 forms of state entries that the native step kernels take (include/cbgx.h), by the key they are kept under; a class
# names the ones its kernels read in ``_step_operands`` ("lig_ptr", the ligand CSR, is built apart: it needs the ligand atoms sorted)
_OPERANDS = {"lig_rows32": ("lig_rows", torch.int32), "gen_l8": ("gen_l", torch.uint8), "lig8": ("lig_flag", torch.uint8),
             "gen8": ("gen_flag", torch.uint8)}


class _Lap:
    """``lap(key)``: add the wall seconds since the previous lap to ``timing[key]`` after a device synchronisation; a no-op
    without a timing dict."""

    def __init__(self, timing, dev):
        self.timing, self.dev = timing, dev
        if timing is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            self.t = time.perf_counter()

    def __call__(self, key):
        if self.timing is None:
            return
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.timing[key] = self.timing.get(key, 0.0) + (now - self.t)
        self.t = now


class BatchesInFlight:
    """``sample_many`` for the sampler classes (TargetDiff, DiffBP, DiffSBDD): ``[self.sample(b) for b in batches]`` with the batches
    IN FLIGHT TOGETHER, round-robin over ``streams`` HIP streams.  The batches are independent (the pocket loop of sample.py:159),
    and while one batch sits in its matrix-bound edge kernel the HBM-bound node kernels and the small kernels of the others fill what
    it leaves (measured +5.5 % with three 200-graph batches).  Each batch's steps stay ordered on its own stream.  With
    ``noise_tapes`` (one per batch, in the form the class's ``sample`` takes) the trajectories equal ``sample``'s bit for bit; without,
    the torch generator is consumed step by step across the batches instead of batch by batch, i.e. the same distribution under a
    different assignment of the draws.  The hooks ``_many_begin(batch, tape, noise) -> state``, ``_many_step(state, t, tape)`` and
    ``_many_finish(state, device) -> trajectory`` default to a class whose tape is a dict t -> that step's noise and whose trajectory is
    its slots (TargetDiff, DiffBP).

    The class also holds what the three ``begin_sampling`` / ``denoise_step`` have in common (the module's docstring).  A class names the
    operands of its native step kernels in ``_step_operands`` and says in ``_counter_refused(st)`` why a state cannot run counter noise."""

    _step_operands = ()

    # ---- static per-batch structure ------------------------------------------------------------
    @staticmethod
    def compose_plan(batch_idx_lig, batch_idx_rec, n_graphs=None):
        """compose_context (repo/modules/common.py:189-214): cat(rec, lig) + stable sort by graph id.
        Returns (sort_idx, batch_idx, lig_rows, graph_ptr); computed once per batch."""
        n_rec, n_lig = batch_idx_rec.shape[0], batch_idx_lig.shape[0]
        if (n_graphs is not None and batch_idx_rec.is_cuda and batch_idx_rec.dtype == torch.int64 and batch_idx_lig.dtype == torch.int64
                and 0 < n_graphs <= (1 << 20) and n_rec + n_lig > 0 and os.environ.get("CBGX_FUSED_COMPOSE", "1") != "0"):
            # the same five results from a counting sort in three launches (csrc/train_embed.hip, cbgx_compose_plan) instead of ~20
            dev = batch_idx_rec.device
            N = n_rec + n_lig
            sort_idx = torch.empty(N, dtype=torch.int64, device=dev)
            batch_idx = torch.empty(N, dtype=torch.int64, device=dev)
            lig_flag = torch.empty(N, dtype=torch.bool, device=dev)
            lig_rows = torch.empty(n_lig, dtype=torch.int64, device=dev)
            graph_ptr = torch.empty(n_graphs + 1, dtype=torch.int32, device=dev)
            scratch = torch.empty(4 * n_graphs + 1, dtype=torch.int32, device=dev)
            _native.check(_native.lib().cbgx_compose_plan(
                _native.ptr(batch_idx_rec.contiguous()), _native.ptr(batch_idx_lig.contiguous()), n_rec, n_lig, int(n_graphs),
                _native.ptr(scratch), _native.ptr(sort_idx), _native.ptr(batch_idx), _native.ptr(lig_flag), _native.ptr(lig_rows),
                _native.ptr(graph_ptr), _native.current_stream(dev)), "cbgx_compose_plan")
            return sort_idx, batch_idx, lig_flag, lig_rows, graph_ptr
        batch_ctx = torch.cat([batch_idx_rec, batch_idx_lig], 0)
        sort_idx = torch.sort(batch_ctx, stable=True).indices
        batch_idx = batch_ctx[sort_idx]
        n_rec = batch_idx_rec.shape[0]
        lig_flag = sort_idx >= n_rec
        # composed rows of ligand atoms, in ligand order = the inverse permutation's tail (no nonzero(): that synchronises)
        inv = torch.empty_like(sort_idx)
        inv[sort_idx] = torch.arange(sort_idx.numel(), device=sort_idx.device)
        lig_rows = inv[n_rec:]
        return sort_idx, batch_idx, lig_flag, lig_rows, graph_ptr_from_batch(batch_idx, n_graphs)

    # ---- the sampling state ----------------------------------------------------------------------
    def _plan_sampling(self, batch, noise, native, v_rec=None, pocket_order=False):
        """First part of ``begin_sampling``, without a torch draw in it: everything about a batch that follows from its index vectors and
        its pocket -- the composition plan, the flags, the composed x / h with the protein rows of h embedded (``v_rec``: the protein
        features to embed, default the batch's), the ``gen_is_ligand`` promise, and the operands of the native step kernels.
        ``native``: the class's own condition for its native step; where its kernels take the ligand CSR (``lig_ptr`` among
        ``_step_operands``) the ligand atoms must be sorted by graph as well, which is how every collate of the reference lays them out.
        That order is looked at ONCE, and only where something depends on it (the CSR, a ``noise``; ``pocket_order``: DiffSBDD's per-graph
        sums, which want the verdict on the pocket's index vector too, in the same host synchronisation), and the CSR is built once:
        ``st['lig_ptr']``, which ``_attach_noise`` hands on as ``st['noise_ptr']``."""
        x_rec = batch["protein_pos"]
        dev = x_rec.device
        bl, br = batch["ligand_element_batch"], batch["protein_element_batch"]
        gen_l = batch.get("ligand_gen_flag", batch["ligand_lig_flag"]).bool()
        gen_r = batch.get("protein_gen_flag", torch.zeros_like(batch["protein_lig_flag"])).bool()
        n_rec, n_lig = x_rec.shape[0], bl.shape[0]
        B = int(bl.max().item()) + 1
        sort_idx, batch_idx, lig_flag, lig_rows, graph_ptr = self.compose_plan(bl, br, B)
        gen_flag = torch.cat([gen_r, gen_l], 0)[sort_idx]
        rec_rows = torch.nonzero(~lig_flag).flatten()
        x = torch.empty(n_rec + n_lig, 3, dtype=torch.float32, device=dev)
        h = torch.empty(n_rec + n_lig, self.context_embedder.emb_dim, dtype=torch.float32, device=dev)
        if v_rec is None:
            v_rec = batch["protein_atom_feature"].float()
        h[rec_rows] = self.context_embedder.embed_protein(v_rec, F.one_hot(batch["protein_aa_type"], NUM_AA).float())    # step-invariant
        st = {"B": B, "N": n_rec + n_lig, "n_lig": n_lig, "x": x, "h": h, "bl": bl, "br": br, "gen_l": gen_l, "batch_idx": batch_idx,
              "lig_flag": lig_flag, "gen_flag": gen_flag, "lig_rows": lig_rows, "rec_rows": rec_rows, "graph_ptr": graph_ptr,
              "traj_x": None, "traj_c": None, "static_h": None, "step_cache": None}
        # every movable row is a ligand row: the h2x blocks fold the query in the edge kernel (CBGX_FWD_GEN_IS_LIGAND)
        st["gen_is_ligand"] = not bool(gen_r.any())
        csr = "lig_ptr" in self._step_operands
        if pocket_order:
            st["bl_sorted"], st["br_sorted"] = torch.stack([(bl[1:] >= bl[:-1]).all(), (br[1:] >= br[:-1]).all()]).tolist()
        elif noise is not None or (native and csr):
            st["bl_sorted"] = bool((bl[1:] >= bl[:-1]).all())
        st["native"] = bool(native and (st["bl_sorted"] if csr else True))
        if st.get("bl_sorted") and (noise is not None or (st["native"] and csr)):
            st["lig_ptr"] = _noise.ligand_csr(bl, B)
        if st["native"]:
            for key in self._step_operands:
                if key != "lig_ptr":
                    src, dtype = _OPERANDS[key]
                    st[key] = st[src].to(dtype).contiguous()
        return st

    def _finish_state(self, st, x_lig, c_lig, x_rec, keep_trajectory, static_cache, noise=None):
        """Second part of ``begin_sampling``, once the initial ligand state and the pocket's positions are known: the protein rows of x,
        the denoiser's static-context cache (the protein rows of (x, h) are the same in all T denoiser calls: the ligand-free first two
        layers, the pocket's neighbour lists and gate values are computed once), the trajectory buffers, and the operands of ``noise``
        unless the class has attached it already."""
        dev, T, rec_rows = st["x"].device, self.num_diffusion_timesteps, st["rec_rows"]
        st["x"][rec_rows] = x_rec
        st["x_lig"], st["c_lig"] = x_lig.contiguous(), c_lig.contiguous()
        if dev.type == "cuda" and static_cache and st["gen_is_ligand"]:
            st["static_h"] = self.denoiser.static_context(x_rec, st["h"][rec_rows], st["br"], rec_rows, st["N"])
            # the node stage and the outputs of layers 0 / 1 from step to step: a fresh block with every static context
            st["step_cache"] = None if st["static_h"] is None else self.denoiser.new_step_cache(st["N"], dev)
        if keep_trajectory:
            # slot s+1 holds the state entering step s; slot 0 = final state (key -1 of the reference's dict)
            st["traj_x"] = torch.empty(T + 1, st["n_lig"], 3, dtype=torch.float32, device=dev)
            st["traj_c"] = torch.empty(T + 1, st["n_lig"], self.num_classes, dtype=torch.float32, device=dev)
            st["traj_x"][T], st["traj_c"][T] = x_lig, c_lig
        if noise is not None and st.get("noise") is None:
            self._attach_noise(st, noise)
        return st

    def _counter_refused(self, st):
        """why ``st`` cannot run counter noise (the kernels that generate it are the native step's), or None"""
        return None

    def _attach_noise(self, st, noise):
        """the operands of the counter mode into a state of ``_plan_sampling``, with the CSR and the verdict it has"""
        why_not = self._counter_refused(st)
        if why_not is not None:
            raise ValueError(why_not)
        _noise.attach(st, noise, st["bl"], st["B"], lig_ptr=st.get("lig_ptr"), ordered=st.get("bl_sorted"))

    def _adopt_noise(self, st, noise):
        """a ``CounterNoise`` given to ``denoise_step``: the state's own from here on if it has none yet, else it must be that one"""
        if st.get("noise") is None:
            self._attach_noise(st, noise)
        elif st["noise"] is not noise:
            raise ValueError("denoise_step: the state already runs on another CounterNoise")

    def _run_denoiser(self, st, need_h=True, h_on_sources=False, workspace=None):
        """the denoiser on the composed arrays of the state -> (x', h', logits)"""
        return self.denoiser(x=st["x"], h=st["h"], batch_idx=st["batch_idx"], lig_flag=st["lig_flag"], gen_flag=st["gen_flag"],
                             graph_ptr=st["graph_ptr"], need_h=need_h, static_h=st["static_h"], workspace=workspace,
                             h_on_sources=h_on_sources, gen_is_ligand=st["gen_is_ligand"], step_cache=st.get("step_cache"))

    def _trajectory(self, st, out_dev, final=None):
        """the returned structure ``traj[t] = (pos, type_onehot, batch_idx)`` for t = T-1 .. -1 from the slots kept on the device (one
        copy each); ``final`` (DiffSBDD): the (pos, types) of its closing draw, which is what key 0 then holds"""
        traj_x, traj_c, bl_out = st["traj_x"].to(out_dev), st["traj_c"].to(out_dev), st["bl"].to(out_dev)
        traj = {t - 1: (traj_x[t], traj_c[t], bl_out) for t in range(self.num_diffusion_timesteps + 1)}
        if final is not None:
            traj[0] = (final[0].to(out_dev), final[1].to(out_dev), bl_out)
        return traj

    # ---- one batch after the other, and several in flight ----------------------------------------------------------------------
    def _begin(self, batch, noise, replay):
        """``begin_sampling`` for ``sample`` / ``sample_many`` of TargetDiff and DiffBP: a replayed tape switches the batch's own
        CounterNoise off"""
        if replay:
            batch = {k: v for k, v in batch.items() if k != "noise_keys"}
        return self.begin_sampling(batch, keep_trajectory=True, noise=None if replay else noise)

    def _many_begin(self, batch, tape, noise=None):
        return self._begin(batch, noise, tape is not None)

    def _many_step(self, st, t_idx, tape):
        self.denoise_step(st, t_idx, tape[t_idx] if tape is not None else None)

    def _many_finish(self, st, out_dev):
        return self._trajectory(st, out_dev)

    def _sample_loop(self, batch, tape, noise, return_device):
        """``sample`` through the hooks: begin, T-1 .. 0, trajectory to ``return_device`` (default: CPU, like the reference)"""
        st = self._many_begin(batch, tape, noise)
        for t_idx in reversed(range(self.num_diffusion_timesteps)):
            self._many_step(st, t_idx, tape)
        return self._many_finish(st, torch.device("cpu") if return_device is None else torch.device(return_device))

    def _side_streams(self, dev, n):
        """the model's own side streams, created once per device: the denoiser keeps one workspace per stream (gigabytes at 100 k
        nodes) and libcbgx one auxiliary stream per caller stream, so the handles must not change from call to call"""
        pool = self.__dict__.setdefault("_stream_pool", {})
        have = pool.setdefault(str(dev), [])
        while len(have) < n:
            have.append(torch.cuda.Stream(dev))
        return have[:n]

    @torch.no_grad()
    def sample_many(self, batches, noise_tapes=None, return_device=None, streams=3, use_graph=False, noise_log=None, timing=None,
                    noise=None):
        """``noise``: one ``CounterNoise`` per batch (or None: the one each batch carries as ``noise_keys``, else the torch
        generator) -- the counter mode, in which the trajectories do not depend on ``streams``, on ``use_graph`` or on which batches
        are in flight together (cbgbench_amd/noise.py).  Not together with ``noise_tapes``.
        ``use_graph`` (classes with ``make_step_graph``; ignored with ``noise_tapes``): every batch's step is captured once as a
        hipGraph on its stream and replayed T times -- one host call per batch and step instead of ~50 launches plus the Python
        around them.  This is what SMALL batches need (the reference's own 10 graphs per batch, sample.py:177-183): one such batch
        is a chain of ~50 dependent 20 us kernels that leaves most of the chip idle, and the host cannot feed eight of them at once;
        eight graphs in flight can.  Same kernels on the same data as the stream launches: identical trajectories
        for identical noise.  ``noise_log`` (tests): a list that receives ``(batch index, t, eps, u)`` after every replay (which
        synchronises the stream).  ``timing`` (a dict): the wall seconds of the three parts of the call are ADDED to its keys
        ``begin_sampling_s`` (static context of every batch), ``steps_s`` (the T steps) and ``traj_download_s`` (trajectory to
        ``return_device``) -- three device synchronisations per call."""
        dev = batches[0]["ligand_pos"].device
        lap = _Lap(timing, dev)
        out_dev = torch.device("cpu") if return_device is None else torch.device(return_device)
        tape = lambda k: None if noise_tapes is None else noise_tapes[k]
        if noise is not None and noise_tapes is not None:
            raise ValueError("sample_many: noise= (counter mode) and noise_tapes (replay) exclude each other")
        if noise is not None and len(noise) != len(batches):
            raise ValueError(f"sample_many: {len(noise)} noise entries for {len(batches)} batches")
        cn = lambda k: None if noise_tapes is not None else _noise.resolve(None if noise is None else noise[k], batches[k])
        T = self.num_diffusion_timesteps
        graphs = bool(use_graph) and noise_tapes is None and dev.type == "cuda" and hasattr(self, "make_step_graph")
        if dev.type != "cuda" or ((len(batches) == 1 or streams <= 1) and not graphs):
            out = []
            for k, b in enumerate(batches):
                st = self._many_begin(b, tape(k), cn(k))
                lap("begin_sampling_s")
                for t_idx in reversed(range(T)):
                    self._many_step(st, t_idx, tape(k))
                lap("steps_s")
                out.append(self._many_finish(st, out_dev))
                lap("traj_download_s")
            return out
        states = [self._many_begin(b, tape(k), cn(k)) for k, b in enumerate(batches)]
        lap("begin_sampling_s")
        cur = torch.cuda.current_stream(dev)
        side = self._side_streams(dev, max(1, min(streams, len(states))))
        for sx in side:
            sx.wait_stream(cur)                      # the states were built on the caller's stream
        if graphs:
            made = [self.make_step_graph(st, stream=side[k % len(side)]) for k, st in enumerate(states)]
            for n in range(T):
                for k, (st, (replay, done)) in enumerate(zip(states, made)):
                    if n < T - done:
                        with torch.cuda.stream(side[k % len(side)]):
                            replay()
                            if noise_log is not None and st.get("_noise") is not None:    # (counter mode has no noise buffers to log)
                                side[k % len(side)].synchronize()
                                noise_log.append((k, T - 1 - done - n, st["_noise"][0].clone(), st["_noise"][1].clone()))   # (torch mode)
        else:
            for t_idx in reversed(range(T)):
                for k, st in enumerate(states):
                    with torch.cuda.stream(side[k % len(side)]):
                        self._many_step(st, t_idx, tape(k))
        for sx in side:
            cur.wait_stream(sx)
        lap("steps_s")
        out = [self._many_finish(st, out_dev) for st in states]
        lap("traj_download_s")
        return out
