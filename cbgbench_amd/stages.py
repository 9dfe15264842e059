"""Thin Python wrappers over the per-stage C-ABI entry points (include/cbgx.h).  The denoiser itself
uses the single ``cbgx_unitransformer_forward`` call; these exist so parity tests (and anyone porting
a different caller) can exercise each stage against the reference function it replaces."""
import torch

from . import _native


def _stream(t):
    return _native.current_stream(t.device)


def knn_graph(x, graph_ptr, k=32):
    """-> (nbr [N,32] int32, deg [N] int32); torch_cluster.knn_graph at unitransformer.py:80."""
    N = x.shape[0]
    nbr = torch.empty(N, 32, dtype=torch.int32, device=x.device)
    deg = torch.empty(N, dtype=torch.int32, device=x.device)
    rc = _native.lib().cbgx_knn_graph(_native.ptr(x), _native.ptr(graph_ptr), graph_ptr.numel() - 1, N, k,
                                      _native.ptr(nbr), _native.ptr(deg), _stream(x))
    _native.check(rc, "cbgx_knn_graph")
    return nbr, deg


def edge_index_from_nbr(nbr, deg):
    """[2,E] (src=neighbour, dst=centre) in the reference's grouped-by-centre order."""
    N = nbr.shape[0]
    slot = torch.arange(32, device=nbr.device)[None, :].expand(N, 32)
    mask = slot < deg[:, None]
    dst = torch.arange(N, device=nbr.device)[:, None].expand(N, 32)[mask]
    return torch.stack([nbr[mask].long(), dst.long()])


def edge_gate(packed, x, nbr, deg):
    e_w = torch.empty(x.shape[0], 32, dtype=torch.float32, device=x.device)
    rc = _native.lib().cbgx_edge_gate(_native.ptr(packed), _native.ptr(x), _native.ptr(nbr), _native.ptr(deg),
                                      x.shape[0], _native.ptr(e_w), _stream(x))
    _native.check(rc, "cbgx_edge_gate")
    return e_w


def _ws(n, device):
    return torch.empty(_native.lib().cbgx_workspace_bytes(n, 1), dtype=torch.uint8, device=device)


def x2h_attention(packed, layer, x, h, nbr, deg, lig_flag, e_w):
    N = x.shape[0]
    out = torch.empty_like(h)
    ws = _ws(N, x.device)
    rc = _native.lib().cbgx_x2h_attention(_native.ptr(packed), layer, _native.ptr(x), _native.ptr(h),
                                          _native.ptr(nbr), _native.ptr(deg), _native.ptr(lig_flag),
                                          _native.ptr(e_w), N, _native.ptr(out), _native.ptr(ws), ws.numel(),
                                          _stream(x))
    _native.check(rc, "cbgx_x2h_attention")
    return out


def h2x_attention(packed, layer, x, h, nbr, deg, lig_flag, gen_flag, e_w, gen_is_ligand=False):
    """``gen_is_ligand``: CBGX_FWD_GEN_IS_LIGAND (cbgx_h2x_attention_v2)"""
    N = x.shape[0]
    x_out = torch.empty_like(x)
    dx = torch.empty_like(x)
    ws = _ws(N, x.device)
    rc = _native.lib().cbgx_h2x_attention_v2(_native.ptr(packed), layer, _native.ptr(x), _native.ptr(h),
                                             _native.ptr(nbr), _native.ptr(deg), _native.ptr(lig_flag),
                                             _native.ptr(gen_flag), _native.ptr(e_w), N, _native.ptr(x_out),
                                             _native.ptr(dx), _native.FWD_GEN_IS_LIGAND if gen_is_ligand else 0, _native.ptr(ws),
                                             ws.numel(), _stream(x))
    _native.check(rc, "cbgx_h2x_attention")
    return x_out, dx


def classifier(packed, num_layers, num_classes, h):
    N = h.shape[0]
    logits = torch.empty(N, num_classes, dtype=torch.float32, device=h.device)
    ws = _ws(N, h.device)
    rc = _native.lib().cbgx_classifier(_native.ptr(packed), num_layers, num_classes, _native.ptr(h), N,
                                       _native.ptr(logits), _native.ptr(ws), ws.numel(), _stream(h))
    _native.check(rc, "cbgx_classifier")
    return logits


def node_stage(packed, layer, x2h, h, lig_flag, rows=None, q_direct=False, fill=0.0):
    """-> (P [N,640], q [N,128], Qt [N,16,128]) of one attention block's node stage (cbgx_node_stage).  ``rows`` (int32, on the
    device): own columns, q and Qt for the listed rows only.  What the call does not write keeps ``fill``."""
    N = h.shape[0]
    P = torch.full((N, 640), fill, dtype=torch.float32, device=h.device)
    q = torch.full((N, 128), fill, dtype=torch.float32, device=h.device)
    Qt = torch.full((N, 16, 128), fill, dtype=torch.float32, device=h.device)
    n_rows = None if rows is None else torch.tensor([rows.numel()], dtype=torch.int32, device=h.device)
    rc = _native.lib().cbgx_node_stage(_native.ptr(packed), layer, int(bool(x2h)), _native.ptr(h), _native.ptr(lig_flag), N,
                                       _native.ptr(rows), _native.ptr(n_rows), int(bool(q_direct)), _native.ptr(P),
                                       _native.ptr(q), _native.ptr(Qt), _stream(h))
    _native.check(rc, "cbgx_node_stage")
    return P, q, Qt


def unitransformer_forward(packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, static=None, graph_part=True,
                           want_h=True, h_on_sources=False, ws=None, fill=None, gen_is_ligand=False):
    """-> (x_out, h_out or None, logits): cbgx_unitransformer_forward, or with ``static`` (the tuple of
    ``UniTransformer.static_context``) cbgx_unitransformer_forward_cached -- ``graph_part=False`` hands over the static features only.
    ``want_h=False``: h_out is NULL; ``h_on_sources``: CBGX_FWD_H_ON_SOURCES; ``gen_is_ligand``: CBGX_FWD_GEN_IS_LIGAND.  ``ws`` (uint8, at least cbgx_workspace_bytes(N, B)): the
    caller's workspace, used as it is; ``fill``: what every output holds before the call."""
    N, B = x.shape[0], graph_ptr.numel() - 1
    x_out, h_out = _outputs(fill, x, h)
    logits = torch.empty(N, num_classes, dtype=torch.float32, device=x.device) if fill is None else \
        torch.full((N, num_classes), fill, dtype=torch.float32, device=x.device)
    if not want_h:
        h_out = None
    ws = torch.empty(_native.lib().cbgx_workspace_bytes(N, B), dtype=torch.uint8, device=x.device) if ws is None else ws
    head = (_native.ptr(packed), num_layers, num_classes, _native.ptr(x), _native.ptr(h), _native.ptr(graph_ptr), _native.ptr(lig_flag),
            _native.ptr(gen_flag), N, B)
    tail = (_native.ptr(ws), ws.numel(), _stream(x))
    flags = _native.FWD_GEN_IS_LIGAND if gen_is_ligand else 0
    if static is None:
        if h_on_sources:
            raise ValueError("unitransformer_forward: CBGX_FWD_H_ON_SOURCES is a flag of the cached entry point")
        rc = _native.lib().cbgx_unitransformer_forward_v2(*head, _native.ptr(x_out), _native.ptr(h_out), _native.ptr(logits), flags, *tail)
    else:
        graph = [_native.ptr(t) if graph_part else None for t in static[2:6]]
        rc = _native.lib().cbgx_unitransformer_forward_cached(*head, _native.ptr(static[0]), _native.ptr(static[1]), *graph,
                                                              _native.ptr(x_out), _native.ptr(h_out), _native.ptr(logits),
                                                              flags | (_native.FWD_H_ON_SOURCES if h_on_sources else 0), *tail)
    _native.check(rc, "cbgx_unitransformer_forward")
    return x_out, h_out, logits


def h2x_stack_forward(packed, num_layers, x, h, graph_ptr, lig_flag, gen_flag, ws=None, fill=None, gen_is_ligand=False):
    """-> x_out [N,3] of cbgx_h2x_stack_forward (``packed``: cbgx_pack_h2x_stack).  ``ws`` / ``fill``: as in unitransformer_forward;
    the call leaves its graph stage (the gen_flag rows only) where ``forward_view`` finds nbr / deg / e_w."""
    N, B = x.shape[0], graph_ptr.numel() - 1
    x_out, = _outputs(fill, x)
    ws = torch.empty(_native.lib().cbgx_workspace_bytes(N, B), dtype=torch.uint8, device=x.device) if ws is None else ws
    rc = _native.lib().cbgx_h2x_stack_forward_v2(_native.ptr(packed), num_layers, _native.ptr(x), _native.ptr(h), _native.ptr(graph_ptr),
                                                 _native.ptr(lig_flag), _native.ptr(gen_flag), N, B, _native.ptr(x_out),
                                                 _native.FWD_GEN_IS_LIGAND if gen_is_ligand else 0, _native.ptr(ws), ws.numel(),
                                                 _stream(x))
    _native.check(rc, "cbgx_h2x_stack_forward")
    return x_out


FORWARD_LISTS = ("act", "A1", "A2", "A3", "D1", "S1", "D2", "S2", "all_general", "all_protein", "D2_general", "D2_protein",
                 "A1_general", "A1_protein", "A2_general", "A2_protein")


def forward_view(ws, n_nodes):
    """TEST-ONLY (libcbgx_xcheck.so, include/cbgx_xcheck.h: call inside ``_native.first_generation_kernels(0)``): what the last forward
    call of ``n_nodes`` nodes on the workspace ``ws`` left there, as views into ``ws`` -- {"nbr" [N,32], "deg" [N], "e_w" [N,32],
    "d1flag" [N], "D1flag" [N], "lists": {name of FORWARD_LISTS: (list [N] int32, count [1] int32)}}."""
    import ctypes
    if not hasattr(_native.lib(), "cbgx_debug_forward_view"):
        raise _native.NativeError("forward_view is test-only: libcbgx.so has no cbgx_debug_forward_view; call it inside "
                                  "_native.first_generation_kernels(0), which switches to libcbgx_xcheck.so")
    out = (ctypes.c_void_p * (5 + 2 * len(FORWARD_LISTS)))()
    _native.check(_native.lib().cbgx_debug_forward_view(_native.ptr(ws), n_nodes, out), "cbgx_debug_forward_view")
    base = ws.data_ptr()

    def at(k, count, dtype):
        off = out[k] - base
        nbytes = count * torch.empty(0, dtype=dtype).element_size()
        if off < 0 or off + nbytes > ws.numel():
            raise _native.NativeError(f"cbgx_debug_forward_view: pointer {k} outside the workspace")
        return ws[off:off + nbytes].view(dtype)

    N = n_nodes
    view = {"nbr": at(0, N * 32, torch.int32).view(N, 32), "deg": at(1, N, torch.int32), "e_w": at(2, N * 32, torch.float32).view(N, 32),
            "d1flag": at(3, N, torch.uint8), "D1flag": at(4, N, torch.uint8), "lists": {}}
    for k, name in enumerate(FORWARD_LISTS):
        view["lists"][name] = (at(5 + 2 * k, N, torch.int32), at(6 + 2 * k, 1, torch.int32))
    return view


# ---- backward of single attention blocks (training; include/cbgx.h "training" section) ---------------------
_MLP_SHAPES_X2H = [(128, 340), (128,), (128,), (128,), (128, 128), (128,)] * 2 + \
                  [(128, 128), (128,), (128,), (128,), (128, 128), (128,)]
_MLP_SHAPES_H2X = [(128, 340), (128,), (128,), (128,), (128, 128), (128,)] + \
                  [(128, 340), (128,), (128,), (128,), (16, 128), (16,)] + \
                  [(128, 128), (128,), (128,), (128,), (128, 128), (128,)]


def _train_ws(n, device):
    return torch.empty(_native.lib().cbgx_train_workspace_bytes(n), dtype=torch.uint8, device=device)


def _grad_tensors(shapes, device, fill=None):
    import ctypes
    gs = [torch.empty(s, dtype=torch.float32, device=device) if fill is None else
          torch.full(s, fill, dtype=torch.float32, device=device) for s in shapes]
    arr = (ctypes.c_void_p * len(gs))(*[g.data_ptr() for g in gs])
    return gs, arr


def _outputs(fill, *like):
    return [torch.empty_like(t) if fill is None else torch.full_like(t, fill) for t in like]


def x2h_attention_backward(packed, layer, x, h, nbr, deg, lig_flag, e_w, grad_h_out, ws=None, fill=None):
    """-> (grad_h, grad_x, grad_e_w, [18 parameter gradients: hk_func(6), hv_func(6), hq_func(6)]).  ``ws`` (uint8, at least
    cbgx_train_workspace_bytes(N)): the caller's workspace, used as it is; ``fill``: what every output holds before the call."""
    N = x.shape[0]
    gh, gx, gew = _outputs(fill, h, x, e_w)
    grads, arr = _grad_tensors(_MLP_SHAPES_X2H, x.device, fill)
    ws = _train_ws(N, x.device) if ws is None else ws
    rc = _native.lib().cbgx_x2h_attention_backward(
        _native.ptr(packed), layer, _native.ptr(x), _native.ptr(h), _native.ptr(nbr), _native.ptr(deg),
        _native.ptr(lig_flag), _native.ptr(e_w), N, _native.ptr(grad_h_out.contiguous()), _native.ptr(gh),
        _native.ptr(gx), _native.ptr(gew), arr, _native.ptr(ws), ws.numel(), _stream(x))
    _native.check(rc, "cbgx_x2h_attention_backward")
    return gh, gx, gew, grads


def h2x_attention_backward(packed, layer, x, h, nbr, deg, lig_flag, gen_flag, e_w, grad_x_out, ws=None, fill=None):
    """-> (grad_h, grad_x, grad_e_w, [18 parameter gradients: xk_func(6), xv_func(6), xq_func(6)]).  ``ws`` / ``fill``: as in
    x2h_attention_backward."""
    N = x.shape[0]
    gh, gx, gew = _outputs(fill, h, x, e_w)
    grads, arr = _grad_tensors(_MLP_SHAPES_H2X, x.device, fill)
    ws = _train_ws(N, x.device) if ws is None else ws
    rc = _native.lib().cbgx_h2x_attention_backward(
        _native.ptr(packed), layer, _native.ptr(x), _native.ptr(h), _native.ptr(nbr), _native.ptr(deg),
        _native.ptr(lig_flag), _native.ptr(gen_flag), _native.ptr(e_w), N, _native.ptr(grad_x_out.contiguous()),
        _native.ptr(gh), _native.ptr(gx), _native.ptr(gew), arr, _native.ptr(ws), ws.numel(), _stream(x))
    _native.check(rc, "cbgx_h2x_attention_backward")
    return gh, gx, gew, grads


_MLP_SHAPES_GATE = [(160, 20), (160,), (160,), (160,), (1, 160), (1,)]


def gate_backward(packed, x, nbr, deg, de_w, rows=None, grad_x=None, ws=None, fill=None):
    """TEST-ONLY (libcbgx_xcheck.so, include/cbgx_xcheck.h: call inside ``_native.first_generation_kernels(0)``): the distance gate's
    backward on ``de_w`` = dL/de_w [N,32] -> [6 gradients of dist_emb.1].  ``rows`` (int32, on the device): walk the listed nodes only;
    ``grad_x`` [N,3]: the gate's coordinate gradient is ADDED to it."""
    N = x.shape[0]
    if not hasattr(_native.lib(), "cbgx_debug_gate_backward"):
        raise _native.NativeError("gate_backward is test-only: libcbgx.so has no cbgx_debug_gate_backward; call it inside "
                                  "_native.first_generation_kernels(0), which switches to libcbgx_xcheck.so")
    grads, arr = _grad_tensors(_MLP_SHAPES_GATE, x.device, fill)
    ws = _train_ws(N, x.device) if ws is None else ws
    n_rows = None if rows is None else torch.tensor([rows.numel()], dtype=torch.int32, device=x.device)
    rc = _native.lib().cbgx_debug_gate_backward(
        _native.ptr(packed), _native.ptr(x), _native.ptr(nbr), _native.ptr(deg), N, _native.ptr(de_w.contiguous()), _native.ptr(rows),
        _native.ptr(n_rows), arr, _native.ptr(grad_x), _native.ptr(ws), ws.numel(), _stream(x))
    _native.check(rc, "cbgx_debug_gate_backward")
    return grads
