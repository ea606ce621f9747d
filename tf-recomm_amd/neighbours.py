"""Nearest neighbours in factor space (include/tfrecomm.h tfr_neighbours): the argument handling the models'
``similar_items`` / ``similar_users`` / ``similar_features`` methods share.  The scoring runs on the device; nothing here
touches a table."""
import numpy as np

from . import _lib as L

METRICS = tuple(L.NB_METRIC)


def metric_code(metric):
    try:
        return L.NB_METRIC[metric]
    except (KeyError, TypeError):
        raise ValueError("metric must be one of %s (got %r)" % (", ".join(METRICS), metric)) from None


def query_host(call, rows, n_rows, k=10, metric="cosine", exclude=None, lo=0, hi=None, return_scores=True, what="row ids"):
    """``call(metric, rows_ptr, n, k, indptr_ptr, excl_ptr, lo, hi, ids_ptr, scores_ptr)`` on host arrays: the ``k`` nearest
    rows of each of ``rows`` among rows ``[lo, hi)`` of an ``n_rows``-row table.  ``exclude``: None or what
    ``engine.exclusion_csr`` takes, row ids of the same table.  Returns ``ids`` int32 ``[n, k]`` (-1 past the eligible rows)
    and, if asked, ``scores`` float32 ``[n, k]`` (-inf there)."""
    from .engine import exclusion_csr
    r = L.as_i32(rows, what).reshape(-1)
    indptr, excl = exclusion_csr(exclude, r)
    ids = np.empty((r.size, int(k)), np.int32)
    scores = np.empty((r.size, int(k)), np.float32) if return_scores else None
    call(metric_code(metric), L.ptr_i32(r), r.size, int(k), None if indptr is None else L.ptr_i64(indptr),
         None if excl is None else L.ptr_i32(excl), int(lo), int(n_rows if hi is None else hi), L.ptr_i32(ids),
         None if scores is None else L.ptr_f32(scores))
    return (ids, scores) if return_scores else ids


def query_dev(call, rows, n_rows, k=10, metric="cosine", exclude=None, lo=0, hi=None, return_scores=True):
    """The same on torch device tensors (``rows`` int32; ``exclude`` None or an (indptr int64, ids int32) pair of device
    tensors aligned with ``rows``).  ``call`` takes the raw pointers and is expected to order itself with torch's stream."""
    import torch
    rows = rows.contiguous()
    if rows.dtype != torch.int32 or rows.dim() != 1:
        raise TypeError("rows must be a 1-D int32 tensor")
    n, k = rows.numel(), int(k)
    ids = torch.empty((n, k), dtype=torch.int32, device=rows.device)
    scores = torch.empty((n, k), dtype=torch.float32, device=rows.device) if return_scores else None
    ip = ex = None
    if exclude is not None:
        ip, ex = exclude[0].contiguous(), exclude[1].contiguous()
        if ip.dtype != torch.int64 or ex.dtype != torch.int32 or ip.numel() != n + 1:
            raise TypeError("exclude must be (indptr int64 [n+1], ids int32) device tensors")
    call(rows.device, metric_code(metric), rows.data_ptr(), n, k, None if ip is None else ip.data_ptr(),
         None if ex is None else ex.data_ptr(), int(lo), int(n_rows if hi is None else hi), ids.data_ptr(),
         None if scores is None else scores.data_ptr())
    return (ids, scores) if return_scores else ids


def plan(dim, k, n, n_candidates):
    """What the launcher will do for ``n`` query rows against ``n_candidates`` rows (no device needed): a dict of the LDS
    bytes per workgroup, query rows per scoring workgroup, candidate slices and query rows per chunk."""
    import ctypes as C
    lds, rpb, sl, ch = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
    L.check(L.load().tfr_neighbours_plan(int(dim), int(k), int(n), int(n_candidates), C.byref(lds), C.byref(rpb),
                                         C.byref(sl), C.byref(ch)))
    return {"lds_bytes": lds.value, "rows_per_block": rpb.value, "slices": sl.value, "row_chunk": ch.value}
