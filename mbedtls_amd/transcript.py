"""Running handshake hashes on the GPU (tlsrec_transcript_batch_update):
update_checksum / mbedtls_ssl_get_handshake_transcript of library/ssl_tls.c and
mbedtls_ssl_reset_transcript_for_hrr of library/ssl_tls13_generic.c for a batch
of connections whose states live in device memory.  Snapshots are 48-byte
elements written where the next batch call reads its transcript."""
from __future__ import annotations

import numpy as np

from . import _abi
from .batch import _ptr, _stream

STATE, SEG, CONN = _abi.TRANSCRIPT_STATE, _abi.TRANSCRIPT_SEG, _abi.TRANSCRIPT_CONN
RESET, SNAPSHOT, HRR = _abi.TRANSCRIPT_RESET, _abi.TRANSCRIPT_SNAPSHOT, _abi.TRANSCRIPT_HRR
SNAPSHOT_LEN = 48


def new_states(n: int, device="cuda"):
    """n zeroed tlsrec_transcript_state (uint8 tensor of n x 208 on `device`): each needs a RESET first"""
    import torch
    return torch.zeros((n, STATE.itemsize), dtype=torch.uint8, device=device)


def _dev(items, like):
    if isinstance(items, np.ndarray):
        import torch
        items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8).reshape(-1).copy()).to(like.device)
    return items


def _len(x, itemsize=1):
    return 0 if x is None else x.numel() * x.element_size() // itemsize


def batch_update(hash_alg, states, conns, segs, arena, out_arena, status, stream=None, nstates=None, nconns=None):
    """conns / segs: CONN / SEG arrays (numpy, or their bytes on the device); states, arena, out_arena:
    uint8 device tensors (arena / out_arena may be None); status: int32 device tensor of nconns.
    Asynchronous on `stream`; raises on a call-level error."""
    nc = (conns.size if isinstance(conns, np.ndarray) else _len(conns, CONN.itemsize)) if nconns is None else nconns
    ns = segs.size if isinstance(segs, np.ndarray) else _len(segs, SEG.itemsize)
    conns, segs = _dev(conns, states), _dev(segs, states)
    r = _abi.load().tlsrec_transcript_batch_update(
        hash_alg, _ptr(states), _len(states, STATE.itemsize) if nstates is None else nstates, _ptr(conns), nc,
        _ptr(segs) if ns else None, ns, _ptr(arena) if _len(arena) else None, _len(arena),
        _ptr(out_arena) if _len(out_arena) else None, _len(out_arena), _ptr(status), _stream(stream))
    if r != 0:
        raise RuntimeError(f"tlsrec_transcript_batch_update failed: {r}")
    return conns, segs       # the device copies, alive until the caller drops them
