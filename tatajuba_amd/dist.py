"""Multi-GPU plumbing: one process per GPU, samples sharded one per rank (the reference's unit of parallelism is the
sample: src/genome_set.c:66-94).  The only exchange on the path is the all-gatherv of the per-sample histograms (the kept
24-byte records) ahead of the cross-sample merge (reference: src/genome_set.c:195-229,250-289).  torch.distributed is
plumbing here: backend "nccl" is RCCL over xGMI on the GPU node, "gloo" in the CPU tests."""
import numpy as np
import torch

RECORD_BYTES = 24


class _DevMem:
    """zero-copy view of device memory owned by the C library"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def device_bytes_tensor(ptr, nbytes, device):
    return torch.as_tensor(_DevMem(ptr, nbytes), device=device)


def all_gatherv_bytes(local, dist, group=None):
    """all-gatherv of a 1-D uint8 tensor: sizes first, then one padded all_gather (xGMI is point-to-point, the payloads
    are MB-scale: one collective on max-padded blocks beats a ring of sends).  Returns (list of tensors, sizes)."""
    world = dist.get_world_size(group)
    if local.is_cuda and dist.get_backend(group) == "gloo":        # rehearsal on a one-GPU box: gloo gathers on the host
        parts, sizes = all_gatherv_bytes(local.cpu(), dist, group)
        return [p.to(local.device) for p in parts], sizes
    n = torch.tensor([local.numel()], dtype=torch.int64, device=local.device)
    sizes_t = torch.empty(world, dtype=torch.int64, device=local.device)
    dist.all_gather_into_tensor(sizes_t, n, group=group)
    sizes = [int(x) for x in sizes_t.tolist()]              # the one host synchronisation of the exchange
    mx = max(max(sizes), 1)
    pad = torch.zeros(mx, dtype=torch.uint8, device=local.device)
    pad[: local.numel()] = local
    out = torch.empty(world * mx, dtype=torch.uint8, device=local.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    return [out[r * mx: r * mx + sz] for r, sz in enumerate(sizes)], sizes


def all_gather_histograms(counter, dist, group=None):
    """Gather every rank's kept records (device-resident, straight from the library's buffer).
    Returns (uint8 tensor of all records concatenated in rank order, list of record counts)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = counter.n_kept
    local = device_bytes_tensor(counter.kept_device_ptr, n * RECORD_BYTES, dev) if n else torch.empty(0, dtype=torch.uint8, device=dev)
    parts, sizes = all_gatherv_bytes(local, dist, group)
    return torch.cat(parts), [s // RECORD_BYTES for s in sizes]


def merge_histograms_device(counter, records_u8, counts):
    """Context-keyed union on the GPU (tjamd_merge_samples): records_u8 = CUDA uint8 tensor holding the samples' kept
    records back to back, counts = records per sample.  Returns (keys uint8 tensor [n_union*24], int32 tensor
    [n_union, n_samples]) in the reference's descending key order."""
    import ctypes as C
    from .capi import lib, TatajubaAmdError, _err
    n = int(sum(counts))
    ns = len(counts)
    keys = torch.empty(max(n, 1) * RECORD_BYTES, dtype=torch.uint8, device=records_u8.device)
    mat = torch.empty((max(n, 1), ns), dtype=torch.int32, device=records_u8.device)
    arr = (C.c_long * ns)(*[int(x) for x in counts])
    torch.cuda.current_stream().synchronize()
    got = lib().tjamd_merge_samples(counter._h, C.c_void_p(records_u8.data_ptr()), arr, ns, C.c_void_p(keys.data_ptr()),
                                    C.c_void_p(mat.data_ptr()), n)
    if got < 0:
        raise TatajubaAmdError(_err())
    return keys[: got * RECORD_BYTES], mat[:got]


def tract_stats_device(counter, keys_u8, mat, coverage, tract_ids=None, ref_length=None, per_sample=True):
    """Per-tract statistics of a union on the GPU (tjamd_tract_stats, then tjamd_tract_sample_stats on the variable tracts):
    keys_u8 / mat as merge_histograms_device returns them, coverage = each sample's coverage, tract_ids / ref_length = CUDA
    int32 tensors (one id per union row / one length per tract) or None.  Returns a dict of numpy arrays: summary
    (TRACT_SUMMARY_DTYPE[n_tracts]), variable (int32 ids, ascending) and, with per_sample, values (float64 [n_var, 5,
    n_samples]), modal_len and n_context (int32 [n_var, n_samples])."""
    import ctypes as C
    import numpy as np
    from .capi import lib, TatajubaAmdError, _err, TRACT_SUMMARY_DTYPE, N_TRACT_STATS
    dev = mat.device
    nu, ns = int(mat.shape[0]), int(mat.shape[1])
    cov = (C.c_int * ns)(*[int(x) for x in coverage])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    summ = torch.empty(max(nu, 1) * TRACT_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    var = torch.empty(max(nu, 1), dtype=torch.int32, device=dev)
    nv = C.c_long()
    torch.cuda.current_stream().synchronize()
    nt = lib().tjamd_tract_stats(counter._h, ptr(keys_u8), ptr(mat), nu, ns, ptr(tract_ids), cov, ptr(ref_length), ptr(summ), ptr(var),
                                 max(nu, 1), C.byref(nv))
    if nt < 0:
        raise TatajubaAmdError(_err())
    out = {"summary": np.frombuffer(summ[: nt * TRACT_SUMMARY_DTYPE.itemsize].cpu().numpy().tobytes(), dtype=TRACT_SUMMARY_DTYPE),
           "variable": var[: nv.value].cpu().numpy()}
    if per_sample:
        n = nv.value
        vals = torch.zeros((max(n, 1), N_TRACT_STATS, ns), dtype=torch.float64, device=dev)
        ml = torch.zeros((max(n, 1), ns), dtype=torch.int32, device=dev)
        nc = torch.zeros((max(n, 1), ns), dtype=torch.int32, device=dev)
        got = lib().tjamd_tract_sample_stats(counter._h, ptr(keys_u8), ptr(mat), nu, ns, cov, ptr(summ), nt, ptr(var), n,
                                             ptr(vals), ptr(ml), ptr(nc))
        if got < 0:
            raise TatajubaAmdError(_err())
        out.update(values=vals[:n].cpu().numpy(), modal_len=ml[:n].cpu().numpy(), n_context=nc[:n].cpu().numpy())
    return out


def union_tracts_device(counter, keys_u8, mat, coverage, max_distance_per_flank, levenshtein_distance, ref_length=None, per_sample=True):
    """Tracts of a union grouped across samples on the GPU (tjamd_union_tracts, tjamd_union_tract_stats, then
    tjamd_union_tract_sample_stats on the selected tracts): keys_u8 / mat as merge_histograms_device returns them, coverage =
    each sample's coverage, ref_length = CUDA int32 tensor (one length per tract) or None.  Returns a dict of numpy arrays:
    tract_id, join_type (int32 per union row), tracts (UNION_TRACT_DTYPE[n_tracts]), summary (UNION_TRACT_SUMMARY_DTYPE),
    variable and selected (int32 ids, ascending) and, with per_sample, values (float64 [n_sel, 5, n_samples]), modal_len,
    n_context and n_len (int32 [n_sel, n_samples]) of the selected tracts."""
    import ctypes as C
    import numpy as np
    from .capi import lib, TatajubaAmdError, _err, UNION_TRACT_DTYPE, UNION_TRACT_SUMMARY_DTYPE, N_TRACT_STATS
    dev = mat.device
    nu, ns = int(mat.shape[0]), int(mat.shape[1])
    cov = (C.c_int * ns)(*[int(x) for x in coverage])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m = max(nu, 1)
    ids = torch.empty(m, dtype=torch.int32, device=dev)
    jt = torch.empty(m, dtype=torch.int32, device=dev)
    tr = torch.empty(m * UNION_TRACT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.current_stream().synchronize()
    nt = lib().tjamd_union_tracts(counter._h, ptr(keys_u8), ptr(mat), nu, ns, int(max_distance_per_flank), int(levenshtein_distance),
                                  ptr(ids), ptr(jt), ptr(tr), m)
    if nt < 0:
        raise TatajubaAmdError(_err())
    summ = torch.empty(max(nt, 1) * UNION_TRACT_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    var = torch.empty(max(nt, 1), dtype=torch.int32, device=dev)
    sel = torch.empty(max(nt, 1), dtype=torch.int32, device=dev)
    nv, nsel = C.c_long(), C.c_long()
    got = lib().tjamd_union_tract_stats(counter._h, ptr(keys_u8), ptr(mat), nu, ns, ptr(tr), nt, cov, ptr(ref_length), ptr(summ),
                                        ptr(var), C.byref(nv), ptr(sel), C.byref(nsel))
    if got < 0:
        raise TatajubaAmdError(_err())
    raw = lambda t, dt, n: np.frombuffer(t[: n * dt.itemsize].cpu().numpy().tobytes(), dtype=dt)
    out = {"tract_id": ids[:nu].cpu().numpy(), "join_type": jt[:nu].cpu().numpy(), "tracts": raw(tr, UNION_TRACT_DTYPE, nt),
           "summary": raw(summ, UNION_TRACT_SUMMARY_DTYPE, nt), "variable": var[: nv.value].cpu().numpy(), "selected": sel[: nsel.value].cpu().numpy()}
    if per_sample:
        n = nsel.value
        vals = torch.zeros((max(n, 1), N_TRACT_STATS, ns), dtype=torch.float64, device=dev)
        ml, nc, nl = (torch.zeros((max(n, 1), ns), dtype=torch.int32, device=dev) for _ in range(3))
        got = lib().tjamd_union_tract_sample_stats(counter._h, ptr(keys_u8), ptr(mat), nu, ns, cov, ptr(summ), nt, ptr(sel), n,
                                                   ptr(vals), ptr(ml), ptr(nc), ptr(nl))
        if got < 0:
            raise TatajubaAmdError(_err())
        out.update(values=vals[:n].cpu().numpy(), modal_len=ml[:n].cpu().numpy(), n_context=nc[:n].cpu().numpy(), n_len=nl[:n].cpu().numpy())
    return out


def located_tracts_device(counter, reference, keys_u8, mat, max_mismatches, tracts=None):
    """A union located on a reference genome and its tracts merged by location on the GPU (tjamd_locate, then
    tjamd_located_tracts): keys_u8 / mat as merge_histograms_device returns them, reference = a capi.Reference of the
    counter's k, tracts = the uint8 CUDA tensor of tjamd_union_tract that union_tracts_device's call fills (or a numpy
    UNION_TRACT_DTYPE array), None for the context-keyed tracts.  Returns a dict: n_located, loc (LOCATION_DTYPE per union
    row), perm (int32), tracts (UNION_TRACT_DTYPE), tract_loc (LOCATION_DTYPE per tract), and the CUDA tensors keys, mat
    (the permuted union), tracts_dev and ref_length (int32 per tract) that tjamd_union_tract_stats takes."""
    import ctypes as C
    import numpy as np
    from .capi import lib, TatajubaAmdError, _err, UNION_TRACT_DTYPE, LOCATION_DTYPE
    dev = mat.device
    nu, ns = int(mat.shape[0]), int(mat.shape[1])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m = max(nu, 1)
    if isinstance(tracts, np.ndarray):
        tracts = torch.from_numpy(np.frombuffer(tracts.astype(UNION_TRACT_DTYPE).tobytes(), dtype=np.uint8).copy()).to(dev)
    nt_in = 0 if tracts is None else tracts.numel() // UNION_TRACT_DTYPE.itemsize
    loc = torch.empty(m * LOCATION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    perm = torch.empty(m, dtype=torch.int32, device=dev)
    okeys = torch.empty_like(keys_u8)
    omat = torch.empty_like(mat)
    otr = torch.empty(m * UNION_TRACT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    tloc = torch.empty(m * LOCATION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rlen = torch.empty(m, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()
    n_located = lib().tjamd_locate(counter._h, reference._h, ptr(keys_u8), nu, int(max_mismatches), ptr(loc))
    if n_located < 0:
        raise TatajubaAmdError(_err())
    nt = lib().tjamd_located_tracts(counter._h, ptr(keys_u8), ptr(mat), nu, ns, ptr(tracts), nt_in, ptr(loc), ptr(perm), ptr(okeys), ptr(omat),
                                    ptr(otr), ptr(tloc), ptr(rlen), m)
    if nt < 0:
        raise TatajubaAmdError(_err())
    raw = lambda t, dt, n: np.frombuffer(t[: n * dt.itemsize].cpu().numpy().tobytes(), dtype=dt)
    return {"n_located": int(n_located), "loc": raw(loc, LOCATION_DTYPE, nu), "perm": perm[:nu].cpu().numpy(), "tracts": raw(otr, UNION_TRACT_DTYPE, nt),
            "tract_loc": raw(tloc, LOCATION_DTYPE, nt), "keys": okeys, "mat": omat, "tracts_dev": otr[: nt * UNION_TRACT_DTYPE.itemsize], "ref_length": rlen[:nt]}
