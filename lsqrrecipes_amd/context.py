"""Context: object wrapper over one lsqr_ctx of the C ABI (one device, one stream)."""
import ctypes as C

import numpy as np

from . import _lib as L


class Context:
    def __init__(self, device=0):
        self._lib = L.load()
        h = C.c_void_p()
        st = self._lib.lsqr_ctx_create(int(device), C.byref(h))
        if st != L.OK:
            raise L.LsqrError(st, "lsqr_ctx_create(device=%d): %s" % (
                device, self._lib.lsqr_status_string(st).decode()))
        self._h = h
        self.device = device
        self.cfg = None
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsqr_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st, allow_empty=False):
        if st == L.OK or (allow_empty and st == L.EMPTY):
            return st
        raise L.LsqrError(st, "%s (%s)" % (self._lib.lsqr_status_string(st).decode(),
                                           self._lib.lsqr_last_error(self._h).decode()))

    # ---- model / data -------------------------------------------------------------------
    def set_model(self, model, dim=3, delta=0.5, ls_type=L.LS_GEOMETRIC, aux=0.0):
        self.cfg = L.ModelCfg(int(model), int(dim), float(delta), int(ls_type), 0, float(aux))
        self._chk(self._lib.lsqr_set_model(self._h, C.byref(self.cfg)))
        self.K = self._lib.lsqr_min_subset(C.byref(self.cfg))
        self.P = self._lib.lsqr_num_params(C.byref(self.cfg))
        self.ND = self._lib.lsqr_record_doubles(C.byref(self.cfg))
        return self

    def upload(self, data):
        a = np.ascontiguousarray(data, dtype=np.float64)
        a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, self.ND)
        self._chk(self._lib.lsqr_upload(self._h, L.ptr(a), a.shape[0], a.shape[1] * 8))
        self.n = a.shape[0]
        self._keep = None  # an upload replaces an attach: the attached memory is the caller's again
        return self

    def attach(self, device_ptr, count, stride_bytes, keepalive=None):
        self._keep = keepalive
        self._chk(self._lib.lsqr_attach(self._h, C.c_void_p(device_ptr), count, stride_bytes))
        self.n = count
        return self

    # ---- hypotheses ---------------------------------------------------------------------
    def hypotheses_from_subsets(self, subsets):
        s = np.ascontiguousarray(subsets, dtype=np.uint32).reshape(-1, self.K)
        self._chk(self._lib.lsqr_hypotheses_from_subsets(self._h, L.ptr(s), s.shape[0]))
        return s.shape[0]

    def hypotheses_sample(self, seed, first, H, want_subsets=False):
        out = np.zeros((H, self.K), dtype=np.uint32) if want_subsets else None
        self._chk(self._lib.lsqr_hypotheses_sample(self._h, seed, first, H, L.ptr(out)))
        return out

    def scan(self):
        self._chk(self._lib.lsqr_scan(self._h))

    def hypotheses(self, params=True, valid=True, votes=True):
        H = self._lib.lsqr_num_hypotheses(self._h)
        p = np.zeros((H, self.P)) if params else None
        v = np.zeros(H, dtype=np.uint8) if valid else None
        c = np.zeros(H, dtype=np.uint32) if votes else None
        self._chk(self._lib.lsqr_get_hypotheses(self._h, L.ptr(p), L.ptr(v), L.ptr(c)))
        return p, v, c

    def hypothesis(self, h):
        p = np.zeros(self.P)
        v = np.zeros(1, dtype=np.uint8)
        self._chk(self._lib.lsqr_get_hypothesis(self._h, int(h), L.ptr(p), L.ptr(v)))
        return p, bool(v[0])

    def best(self):
        packed = C.c_uint64(0)
        self._chk(self._lib.lsqr_best(self._h, C.byref(packed)))
        v = packed.value
        return v, v >> 32, 0xFFFFFFFF - (v & 0xFFFFFFFF)

    # ---- mask / fit ---------------------------------------------------------------------
    def mask(self, params, begin=0, end=None, want_mask=True):
        end = self.n if end is None else end
        p = np.ascontiguousarray(params, dtype=np.float64)
        m = np.zeros(end - begin, dtype=np.uint8) if want_mask else None
        cnt = C.c_uint64(0)
        self._chk(self._lib.lsqr_mask(self._h, L.ptr(p), begin, end, L.ptr(m), C.byref(cnt)))
        return m, cnt.value

    def mask_from_hypothesis(self, h, want_mask=True):
        m = np.zeros(self.n, dtype=np.uint8) if want_mask else None
        cnt = C.c_uint64(0)
        self._chk(self._lib.lsqr_mask_from_hypothesis(self._h, h, L.ptr(m), C.byref(cnt)))
        return m, cnt.value

    def set_mask(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape[0] == self.n
        self._chk(self._lib.lsqr_set_mask(self._h, L.ptr(m)))

    def ls_fit(self, use_mask=False):
        """-> (params ndarray, possibly empty; FitInfo)"""
        out = np.zeros(max(self.P, 32))
        info = L.FitInfo()
        st = self._chk(self._lib.lsqr_ls_fit(self._h, int(use_mask), L.ptr(out), C.byref(info)),
                       allow_empty=True)
        self.last_iterate = out[:self.P].copy()   # LM runs: the last iterate even when the fit is reported failed
        return (out[:info.n_params].copy() if st == L.OK else np.zeros(0)), info

    def moments_len(self, phase):
        return self._lib.lsqr_moments_len(C.byref(self.cfg), phase)

    def moments(self, x, begin=0, end=None, phase=0, use_mask=False):
        end = self.n if end is None else end
        xv = np.zeros(32)
        x = np.asarray(x, dtype=np.float64)
        xv[:len(x)] = x
        blk = np.zeros(self.moments_len(phase))
        self._chk(self._lib.lsqr_moments(self._h, int(use_mask), begin, end, phase, L.ptr(xv),
                                         L.ptr(blk)))
        return blk

    def moments_dev(self, x, block_ptr, begin=0, end=None, phase=0, use_mask=False):
        """moments() with the block left at device address block_ptr, no synchronisation"""
        end = self.n if end is None else end
        xv = np.zeros(32)
        x = np.asarray(x, dtype=np.float64)
        xv[:len(x)] = x
        self._chk(self._lib.lsqr_moments_dev(self._h, int(use_mask), begin, end, phase, L.ptr(xv),
                                             C.c_void_p(block_ptr)))

    def winner_moments(self, seed, stream_index, begin=0, end=None):
        """-> (params, origin(32), block, count): lsqr_winner_moments, one host synchronisation"""
        end = self.n if end is None else end
        par = np.zeros(max(self.P, 1))
        org = np.zeros(32)
        blk = np.zeros(self.moments_len(0))
        cnt = C.c_uint64(0)
        self._chk(self._lib.lsqr_winner_moments(self._h, seed, stream_index, begin, end, L.ptr(par),
                                                L.ptr(org), L.ptr(blk), C.byref(cnt)))
        return par, org, blk, cnt.value

    def solve_moments(self, block, origin):
        b = np.ascontiguousarray(block, dtype=np.float64)
        o = np.zeros(32)
        o[:len(origin)] = origin
        out = np.zeros(max(self.P, 32))
        info = L.FitInfo()
        st = self._chk(self._lib.lsqr_solve_moments(self._h, L.ptr(b), L.ptr(o), L.ptr(out),
                                                    C.byref(info)), allow_empty=True)
        return (out[:info.n_params].copy() if st == L.OK else np.zeros(0)), info

    def lm_begin(self, x0):
        x = np.zeros(32)
        x0 = np.asarray(x0, dtype=np.float64)[:32]
        x[:len(x0)] = x0
        xt = np.zeros(32)
        self._chk(self._lib.lsqr_lm_begin(self._h, L.ptr(x), L.ptr(xt)))
        return xt

    def lm_step(self, block):
        b = np.ascontiguousarray(block, dtype=np.float64)
        xt = np.zeros(32)
        out = np.zeros(max(self.P, 64))
        cont = C.c_int(0)
        info = L.FitInfo()
        st = self._chk(self._lib.lsqr_lm_step(self._h, L.ptr(b), L.ptr(xt), C.byref(cont),
                                              L.ptr(out), C.byref(info)), allow_empty=True)
        return bool(cont.value), xt, (out[:info.n_params].copy() if st == L.OK else np.zeros(0)), info

    def stats(self, params, use_mask=False):
        p = np.ascontiguousarray(params, dtype=np.float64)
        out = np.zeros(4)
        self._chk(self._lib.lsqr_stats(self._h, L.ptr(p), int(use_mask), L.ptr(out)))
        return out

    # ---- multi-GPU step with device-resident exchange buffers ---------------------------
    def set_stream(self, hip_stream):
        """enqueue on the caller's HIP stream (int handle, e.g. torch.cuda.current_stream().cuda_stream;
        0 is the default stream); None restores the context's own stream"""
        if hip_stream is None:
            self._chk(self._lib.lsqr_set_stream(self._h, None, 0))
        else:
            self._chk(self._lib.lsqr_set_stream(self._h, C.c_void_p(int(hip_stream) or None), 1))

    def step_scan(self, seed, first, H, index_base, packed_ptr):
        self._chk(self._lib.lsqr_step_scan(self._h, seed, first, H, index_base, C.c_void_p(packed_ptr)))

    def step_winner(self, seed, batch_first, packed_ptr, begin, end, block_ptr):
        self._chk(self._lib.lsqr_step_winner(self._h, seed, batch_first, C.c_void_p(packed_ptr), begin, end,
                                             C.c_void_p(block_ptr)))

    def step_finish(self, packed_ptr, block_ptr):
        """-> (status, winner params, fitted params (possibly empty), RansacInfo)"""
        win = np.zeros(max(self.P, 1))
        out = np.zeros(max(self.P, 64))
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_step_finish(self._h, C.c_void_p(packed_ptr), C.c_void_p(block_ptr),
                                                  L.ptr(win), L.ptr(out), C.byref(info)), allow_empty=True)
        fit = out[:info.n_params].copy() if st == L.OK else np.zeros(0)
        return st, win, fit, info

    def step_finish_enqueue(self, packed_ptr, block_ptr, slot=0):
        self._chk(self._lib.lsqr_step_finish_enqueue(self._h, C.c_void_p(packed_ptr), C.c_void_p(block_ptr), slot))

    def step_finish_wait(self, slot=0):
        win = np.zeros(max(self.P, 1))
        out = np.zeros(max(self.P, 64))
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_step_finish_wait(self._h, slot, L.ptr(win), L.ptr(out), C.byref(info)),
                       allow_empty=True)
        fit = out[:info.n_params].copy() if st == L.OK else np.zeros(0)
        return st, win, fit, info

    def residuals(self, params, begin=0, end=None):
        """the model's residual of every record in [begin, end) (lsqr_residuals)"""
        end = self.n if end is None else end
        p = np.ascontiguousarray(params, dtype=np.float64)
        out = np.zeros(end - begin)
        self._chk(self._lib.lsqr_residuals(self._h, L.ptr(p), begin, end, L.ptr(out)))
        return out

    # ---- whole path ---------------------------------------------------------------------
    def ransac(self, p, seed=1, subsets=None, want_consensus=True):
        out = np.zeros(max(self.P, 32))
        cons = np.zeros(max(self.n, 1), dtype=np.uint8) if want_consensus else None
        info = L.RansacInfo()
        s = None
        ns = 0
        if subsets is not None:
            s = np.ascontiguousarray(subsets, dtype=np.uint32).reshape(-1, self.K)
            ns = s.shape[0]
        st = self._lib.lsqr_ransac(self._h, float(p), seed, L.ptr(s), ns, L.ptr(out), L.ptr(cons),
                                   C.byref(info))
        if st == L.ERR_INVALID and info.iterations == 0 and info.fraction == 0:
            return dict(status=st, fraction=0.0, params=None, consensus=None, info=info)
        self._chk(st, allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0),
                    consensus=cons[:self.n] if (cons is not None and info.best_votes > 0) else None,
                    info=info)

    def ransac_sequential(self, p, max_models, seeds=None, min_votes=0, want_labels=True):
        """Sequential RANSAC on the current upload / attach (lsqr_ransac_sequential): find a model, take its consensus
        set out, search what is left, up to max_models times, the records staying on the device.  Round r is decided
        as ransac(p, seed=seeds[r]) on a context holding only the records no earlier round claimed (default seeds
        1 + r); a round is accepted when it is OK with best_votes >= max(min_votes, 1), the first one that is not
        ends the call.  -> dict: n_models; params (max_models x P, zero rows where status is not OK); labels (one
        int32 per record in upload order: the round that claimed it, else -1; None unless want_labels); status
        (ERR_STATE for a round that did not run) and, per round, fraction, iterations, best_index, best_votes,
        evaluated, n_params, n_used, lm_info, lm_nfev, cost -- the rejected round's included.  The context holds the
        original records afterwards, as after upload / attach."""
        m = int(max_models)
        if m < 0:
            raise ValueError("max_models must not be negative")
        seeds = (1 + np.arange(m, dtype=np.uint64)) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (m,):
            raise ValueError("one seed per model")
        params = np.zeros((max(m, 1), self.P))
        labels = np.full(max(self.n, 1), -1, dtype=np.int32) if want_labels else None
        infos = (L.RansacInfo * max(m, 1))()
        status = np.full(max(m, 1), L.ERR_STATE, dtype=np.int32)
        n_models = C.c_size_t(0)
        self._chk(self._lib.lsqr_ransac_sequential(self._h, float(p), L.ptr(seeds), m, int(min_votes), L.ptr(params),
                                                   L.ptr(labels), infos, L.ptr(status), C.byref(n_models)))
        status, params = status[:m], params[:m]
        params[status != L.OK] = 0.0
        inf = np.ctypeslib.as_array(infos)[:m]
        f = lambda name: inf[name].copy()
        fit = inf["fit"]
        return dict(n_models=int(n_models.value), params=params, labels=labels[:self.n] if labels is not None else None,
                    status=status, fraction=f("fraction"), iterations=f("iterations"), best_index=f("best_index"),
                    best_votes=f("best_votes"), evaluated=f("evaluated"), n_params=f("n_params"),
                    n_used=fit["n_used"].copy(), lm_info=fit["lm_info"].copy(), lm_nfev=fit["lm_nfev"].copy(),
                    cost=fit["cost"].copy())

    def ransac_many(self, problems, p, seeds=None, want_consensus=True):
        """Many independent RANSAC problems in one call (lsqr_ransac_many) with the context's model: plane, line,
        algebraic sphere, absolute orientation (ls_type 0, or 2 with 7-double weighted records), pivot, ray and 2-D
        line; any other model raises LsqrError(ERR_INVALID).  Records are self.ND doubles wide, as for upload.
        problems: a list of record arrays, or (records, offsets) with problem j = records[offsets[j]:offsets[j+1]].
        seeds: one sampler stream per problem (default 1 + arange(n)); problem j is decided as
        ransac(p, seed=seeds[j]) on its records alone.  -> dict of arrays: status, fraction, iterations,
        best_index, best_votes, evaluated, n_params, n_used, params (n x P, zero rows where status is not OK),
        consensus (flat, aligned with offsets; None unless want_consensus) and offsets."""
        return self._ransac_many(self._lib.lsqr_ransac_many, problems, p, seeds, want_consensus)

    def ransac_many_sequential(self, problems, p, max_models, seeds=None, min_votes=0, want_labels=True):
        """Sequential RANSAC over many independent problems in one call (lsqr_ransac_many_sequential): one upload,
        every round one batched search over the problems still going, their unclaimed records compacted on the device
        in between.  problems as for ransac_many; every model ransac_many, ransac_many_lm or ransac_many_dense takes.
        seeds: (n, max_models), default 1 + j * max_models + r.  Problem j is decided as upload(problem j) +
        ransac_sequential(p, max_models, seeds[j], min_votes).  -> dict: n_models (n,); status and the keys of
        ransac_sequential per round, (n, max_models) (ERR_STATE / zeros for a round that did not run); params
        (n, max_models, P), zero where status is not OK; labels (flat int32, aligned with offsets: the round that
        claimed the record, else -1; None unless want_labels) and offsets."""
        m = int(max_models)
        if m < 0:
            raise ValueError("max_models must not be negative")
        recs, offs = self._many_records(problems)
        n = len(offs) - 1
        if seeds is None:
            seeds = 1 + np.arange(n * m, dtype=np.uint64).reshape(n, m)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (n, m):
            raise ValueError("one seed per problem and model")
        total = int(offs[-1]) if n else 0
        params = np.zeros((max(n * m, 1), self.P))
        labels = np.full(max(total, 1), -1, dtype=np.int32) if want_labels else None
        infos = (L.RansacInfo * max(n * m, 1))()
        status = np.full(max(n * m, 1), L.ERR_STATE, dtype=np.int32)
        n_models = np.zeros(max(n, 1), dtype=np.uintp)
        self._chk(self._lib.lsqr_ransac_many_sequential(self._h, L.ptr(recs), self.ND * 8, L.ptr(offs), n, float(p),
                                                        L.ptr(seeds), m, int(min_votes), L.ptr(params), L.ptr(labels),
                                                        infos, L.ptr(status), L.ptr(n_models)))
        status = status[:n * m].reshape(n, m)
        params = params[:n * m].reshape(n, m, self.P)
        params[status != L.OK] = 0.0
        inf = np.ctypeslib.as_array(infos)[:n * m]
        f = lambda name: inf[name].reshape(n, m).copy()
        fit = inf["fit"]
        g = lambda name: fit[name].reshape(n, m).copy()
        return dict(n_models=n_models[:n].astype(np.int64), params=params,
                    labels=labels[:total] if labels is not None else None, status=status, fraction=f("fraction"),
                    iterations=f("iterations"), best_index=f("best_index"), best_votes=f("best_votes"),
                    evaluated=f("evaluated"), n_params=f("n_params"), n_used=g("n_used"), lm_info=g("lm_info"),
                    lm_nfev=g("lm_nfev"), cost=g("cost"), offsets=offs)

    def ransac_grouped(self, groups, n_groups, p, seeds=None, want_consensus=True, consensus_out=None):
        """One RANSAC problem per label over the records of the current upload / attach (lsqr_ransac_grouped): problem g
        is the records i with groups[i] == g, in upload order; a label that is negative or >= n_groups puts the record
        in no problem.  The records are grouped on the device and never cross to the host.  Every model ransac_many,
        ransac_many_lm or ransac_many_dense takes; problem g is decided, bit for bit, as that call decides it on the
        stable gather by label of the records with seeds[g] (default 1 + arange(n_groups)).
        groups: a numpy integer array (host form), or a device tensor -- anything with data_ptr() and is_cuda, int32,
        contiguous, one entry per record.  For the device form, consensus_out may be a uint8 device tensor of one byte
        per record, which receives the consensus without a copy to the host.
        -> ransac_many's dict plus lm_info, lm_nfev, cost and reserved; offsets: the prefix sums of the group sizes;
        consensus: one byte per record in upload order, 0 for a record in no problem or in a problem without a winner
        -- a numpy array for the host form, the caller's tensor for the device form (None unless want_consensus, or
        where the device form got no consensus_out)."""
        if self.cfg is None:
            raise L.LsqrError(L.ERR_STATE, "set_model has not been called")
        n = int(n_groups)
        if n < 0:
            raise ValueError("n_groups must not be negative")
        total = int(self._lib.lsqr_count(self._h))
        on_device = hasattr(groups, "data_ptr")
        cons = None
        if on_device:
            if not groups.is_cuda or "int32" not in str(groups.dtype) or not groups.is_contiguous():
                raise ValueError("device groups must be a contiguous int32 device tensor")
            if groups.numel() != total:
                raise ValueError("one label per record")
            g_ptr = groups.data_ptr()
            c_ptr = None
            if consensus_out is not None and want_consensus:
                c = consensus_out
                if not (hasattr(c, "data_ptr") and c.is_cuda and "uint8" in str(c.dtype) and c.is_contiguous()
                        and c.numel() == total):
                    raise ValueError("consensus_out must be a contiguous uint8 device tensor of one byte per record")
                cons, c_ptr = c, c.data_ptr()
        else:
            if consensus_out is not None:
                raise ValueError("consensus_out goes with device groups")
            g = np.asarray(groups)
            if g.dtype.kind not in "iu":
                raise ValueError("groups must be integers")
            if g.shape != (total,):
                raise ValueError("one label per record")
            # (labels beyond int32 are in no problem, as -1 is)
            g = np.ascontiguousarray(np.where((g >= 0) & (g <= 0x7FFFFFFF), g, -1) if g.dtype != np.int32 else g,
                                     dtype=np.int32)
            g_ptr = L.ptr(g)
            cons = np.zeros(max(total, 1), dtype=np.uint8) if want_consensus else None
            c_ptr = L.ptr(cons)
        seeds = (1 + np.arange(n, dtype=np.uint64)) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (n,):
            raise ValueError("one seed per group")
        params = np.zeros((max(n, 1), self.P))
        offs = np.zeros(n + 1, dtype=np.uint64)
        infos = (L.RansacInfo * max(n, 1))()
        status = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._lib.lsqr_ransac_grouped(self._h, g_ptr, n, 1 if on_device else 0, float(p), L.ptr(seeds),
                                                L.ptr(params), c_ptr, L.ptr(offs), infos, L.ptr(status)))
        status, params = status[:n], params[:n]
        params[status != L.OK] = 0.0
        inf = np.ctypeslib.as_array(infos)[:n]
        f = lambda name: inf[name].copy()
        fit = inf["fit"]
        if cons is not None and not on_device:
            cons = cons[:total]
        return dict(status=status, fraction=f("fraction"), iterations=f("iterations"), best_index=f("best_index"),
                    best_votes=f("best_votes"), evaluated=f("evaluated"), n_params=f("n_params"),
                    n_used=fit["n_used"].copy(), lm_info=fit["lm_info"].copy(), lm_nfev=fit["lm_nfev"].copy(),
                    cost=fit["cost"].copy(), reserved=fit["reserved"].copy(), params=params, consensus=cons,
                    offsets=offs)

    def ransac_grouped_sequential(self, groups, n_groups, p, max_models, seeds=None, min_votes=0, want_labels=True,
                                  labels_out=None):
        """Several models per label over the records of the current upload / attach (lsqr_ransac_grouped_sequential):
        ransac_grouped's records and labels, ransac_many_sequential's rounds.  Group g is the records i with
        groups[i] == g, in upload order; a label that is negative or >= n_groups puts the record in no group.  The
        records are grouped on the device and never cross to the host.  Every model ransac_many_sequential takes; group
        g is decided, bit for bit, as that call decides problem g of the stable gather by label of the records with
        seeds[g] (seeds: (n_groups, max_models), default 1 + g * max_models + r) and the same max_models, min_votes, p.
        groups: a numpy integer array (host form), or a device tensor -- anything with data_ptr() and is_cuda, int32,
        contiguous, one entry per record.  For the device form, labels_out may be a contiguous int32 device tensor of
        one entry per record, which receives the labels without a copy to the host; nothing is allocated on the device
        here.
        -> ransac_many_sequential's dict (status ERR_STATE / zeros for rounds not run, params zero where status is not
        OK); offsets: the prefix sums of the group sizes; labels: per record in upload order the round that claimed it
        inside its group, -1 for an unclaimed record or one in no group -- a numpy array for the host form, the
        caller's tensor for the device form (None unless want_labels, or where the device form got no labels_out)."""
        if self.cfg is None:
            raise L.LsqrError(L.ERR_STATE, "set_model has not been called")
        n, m = int(n_groups), int(max_models)
        if n < 0:
            raise ValueError("n_groups must not be negative")
        if m < 0:
            raise ValueError("max_models must not be negative")
        total = int(self._lib.lsqr_count(self._h))
        on_device = hasattr(groups, "data_ptr")
        labels = None
        if on_device:
            if not groups.is_cuda or "int32" not in str(groups.dtype) or not groups.is_contiguous():
                raise ValueError("device groups must be a contiguous int32 device tensor")
            if groups.numel() != total:
                raise ValueError("one label per record")
            g_ptr = groups.data_ptr()
            l_ptr = None
            if labels_out is not None and want_labels:
                t = labels_out
                if not (hasattr(t, "data_ptr") and t.is_cuda and "int32" in str(t.dtype) and t.is_contiguous()
                        and t.numel() == total):
                    raise ValueError("labels_out must be a contiguous int32 device tensor of one entry per record")
                labels, l_ptr = t, t.data_ptr()
        else:
            if labels_out is not None:
                raise ValueError("labels_out goes with device groups")
            g = np.asarray(groups)
            if g.dtype.kind not in "iu":
                raise ValueError("groups must be integers")
            if g.shape != (total,):
                raise ValueError("one label per record")
            # (labels beyond int32 are in no group, as -1 is)
            g = np.ascontiguousarray(np.where((g >= 0) & (g <= 0x7FFFFFFF), g, -1) if g.dtype != np.int32 else g,
                                     dtype=np.int32)
            g_ptr = L.ptr(g)
            labels = np.full(max(total, 1), -1, dtype=np.int32) if want_labels else None
            l_ptr = L.ptr(labels)
        if seeds is None:
            seeds = 1 + np.arange(n * m, dtype=np.uint64).reshape(n, m)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (n, m):
            raise ValueError("one seed per group and model")
        params = np.zeros((max(n * m, 1), self.P))
        offs = np.zeros(n + 1, dtype=np.uint64)
        infos = (L.RansacInfo * max(n * m, 1))()
        status = np.full(max(n * m, 1), L.ERR_STATE, dtype=np.int32)
        n_models = np.zeros(max(n, 1), dtype=np.uintp)
        self._chk(self._lib.lsqr_ransac_grouped_sequential(
            self._h, g_ptr, n, 1 if on_device else 0, float(p), L.ptr(seeds), m, int(min_votes), L.ptr(params), l_ptr,
            L.ptr(offs), infos, L.ptr(status), L.ptr(n_models)))
        status = status[:n * m].reshape(n, m)
        params = params[:n * m].reshape(n, m, self.P)
        params[status != L.OK] = 0.0
        inf = np.ctypeslib.as_array(infos)[:n * m]
        f = lambda name: inf[name].reshape(n, m).copy()
        fit = inf["fit"]
        h = lambda name: fit[name].reshape(n, m).copy()
        if labels is not None and not on_device:
            labels = labels[:total]
        return dict(n_models=n_models[:n].astype(np.int64), params=params, labels=labels, status=status,
                    fraction=f("fraction"), iterations=f("iterations"), best_index=f("best_index"),
                    best_votes=f("best_votes"), evaluated=f("evaluated"), n_params=f("n_params"), n_used=h("n_used"),
                    lm_info=h("lm_info"), lm_nfev=h("lm_nfev"), cost=h("cost"), offsets=offs)

    def _assign_args(self, params, labels_out):
        """the rows and the label buffer of assign / refine -> (params (M x P), M, total, on_device, labels, l_ptr)"""
        if self.cfg is None:
            raise L.LsqrError(L.ERR_STATE, "set_model has not been called")
        par = np.array(params, dtype=np.float64, order="C")  # a copy: refine writes it
        par = par.reshape(-1, self.P) if par.size else par.reshape(0, self.P)
        total = int(self._lib.lsqr_count(self._h))
        on_device = labels_out is not None
        if on_device:
            t = labels_out
            if not (hasattr(t, "data_ptr") and t.is_cuda and "int32" in str(t.dtype) and t.is_contiguous()
                    and t.numel() == total):
                raise ValueError("labels_out must be a contiguous int32 device tensor of one entry per record")
            labels, l_ptr = t, t.data_ptr()
        else:
            labels = np.full(max(total, 1), -1, dtype=np.int32)
            l_ptr = L.ptr(labels)
        return par, par.shape[0], total, on_device, labels, l_ptr

    def assign(self, params, want_residuals=False, labels_out=None):
        """Every record of the current upload / attach to the nearest of the models it agrees with (lsqr_assign).
        params: M <= 64 rows of P parameters.  label = the smallest m that minimises residual(params[m], x) among the m
        with agree(params[m], x), -1 when none agrees (and for a record with a non-finite coordinate).  Plane, line,
        sphere (either ls_type) and 2-D line; any other model raises LsqrError(ERR_INVALID).
        labels_out may be a contiguous int32 device tensor of one entry per record -- anything with data_ptr() and
        is_cuda --, which receives the labels without a copy to the host; the residuals then stay on the host side out
        of the call (want_residuals must be False).
        -> dict: labels (int32 per record in upload order; a numpy array, or the caller's tensor), residuals (float64
        per record: the residual to the assigned model, +inf for -1; None unless want_residuals) and counts (uint64,
        M + 1: records per model, then the unassigned ones)."""
        return self._assign(self._lib.lsqr_assign, params, want_residuals, labels_out)

    def _assign(self, call, params, want_residuals, labels_out):
        """lsqr_assign or lsqr_assign_dense -> assign's dict"""
        par, m, total, on_device, labels, l_ptr = self._assign_args(params, labels_out)
        if on_device and want_residuals:
            raise ValueError("want_residuals goes with host labels")
        res = np.full(max(total, 1), np.inf) if want_residuals else None
        counts = np.zeros(m + 1, dtype=np.uint64)
        if m == 0:
            counts[0] = total
        self._chk(call(self._h, L.ptr(par), m, 1 if on_device else 0, l_ptr, L.ptr(res), L.ptr(counts)))
        if not on_device:
            labels = labels[:total]
        return dict(labels=labels, residuals=res[:total] if res is not None else None, counts=counts)

    def refine(self, params, max_rounds=8, labels_out=None):
        """Assignment and least-squares refit in turn, on the device (lsqr_refine): L_r = assign(params_r); stop when
        r > 0 and L_r == L_{r-1} (converged) or r == max_rounds; else params_{r+1} = the fit of every model on its own
        records, r += 1.  A model with fewer than K records, or whose fit gives no result, keeps its row for that round.
        The models of assign, except the geometric sphere (ERR_INVALID).  labels_out as for assign.
        -> dict: params (M x P: params_r), labels (L_r: exactly assign(params)["labels"]), counts (M + 1, of L_r),
        status (OK or EMPTY per model for the last refit round; OK when none ran), n_used (records behind the last
        refit attempt), rounds (refits done) and converged."""
        return self._refine(self._lib.lsqr_refine, params, max_rounds, labels_out)[0]

    def _refine(self, call, params, max_rounds, labels_out):
        """lsqr_refine, lsqr_refine_lm or lsqr_refine_dense -> (refine's dict, the fits as a structured array)"""
        par, m, total, on_device, labels, l_ptr = self._assign_args(params, labels_out)
        if int(max_rounds) < 0:
            raise ValueError("max_rounds must not be negative")
        counts = np.zeros(m + 1, dtype=np.uint64)
        if m == 0:
            counts[0] = total
        fits = (L.FitInfo * max(m, 1))()
        status = np.zeros(max(m, 1), dtype=np.int32)
        rounds, conv = C.c_size_t(0), C.c_int(0)
        self._chk(call(self._h, L.ptr(par), m, int(max_rounds), 1 if on_device else 0, l_ptr, L.ptr(counts), fits,
                       L.ptr(status), C.byref(rounds), C.byref(conv)))
        if not on_device:
            labels = labels[:total]
        f = np.ctypeslib.as_array(fits)[:m]
        return dict(params=par, labels=labels, counts=counts, status=status[:m], n_used=f["n_used"].copy(),
                    rounds=int(rounds.value), converged=bool(conv.value)), f

    def refine_lm(self, params, max_rounds=8, labels_out=None):
        """refine for the sphere with LS_GEOMETRIC, which refine refuses (lsqr_refine_lm): the same loop, and the refit
        of a model is a Levenberg-Marquardt run over its own records from their algebraic fit, on the device, all
        models at once.  A model whose run does not end with lm_info in 1..4 (or that has fewer than K records, or no
        algebraic start) keeps the row it had before the round.  Any other model raises LsqrError(ERR_INVALID).
        -> refine's dict, and per model for the last refit round lm_info, lm_nfev, cost and stall (the evaluation after
        which the cost never again fell by more than 1e-7 relative); zeros where no run started."""
        out, f = self._refine(self._lib.lsqr_refine_lm, params, max_rounds, labels_out)
        out.update(lm_info=f["lm_info"].copy(), lm_nfev=f["lm_nfev"].copy(), cost=f["cost"].copy(),
                   stall=f["reserved"].copy())
        return out

    def assign_dense(self, params, want_residuals=False, labels_out=None):
        """assign for the dense linear system, which assign refuses (lsqr_assign_dense): every row (a | b) of the
        current upload / attach to the nearest of the regressions it agrees with.  params: M <= 64 rows of n
        coefficients.  label = the smallest m that minimises |a . params[m] - b| among the m with
        |a . params[m] - b| < delta, -1 when none agrees (and for a row with a non-finite slot among its n + 1).  The
        dot product is the running sum in slot order, so labels and residuals equal mask() / residuals() of that row
        bit for bit.  Any other model raises LsqrError(ERR_INVALID).  labels_out and the result as for assign."""
        return self._assign(self._lib.lsqr_assign_dense, params, want_residuals, labels_out)

    def refine_dense(self, params, max_rounds=8, labels_out=None):
        """refine for the dense linear system (lsqr_refine_dense): the same loop, and the refit of a regression is the
        least-squares solution over its own rows by ls_fit's route -- the elimination on the Gram block under the
        options dense_fast_solve and dense_dd, the double-double solve from the rows where it meets a pivot below
        1e-6 max|G|.  A regression with fewer than n rows, or whose solve gives no result, keeps its row for that
        round.  Each round reads the rows once.  Any other model raises LsqrError(ERR_INVALID).
        -> refine's dict, and route: per model the route of the last refit round as ls_fit reports it (0: the
        elimination, 1: double-double, 2: dense_dd 0 and a pivot below 1e-6); zeros where none ran."""
        out, f = self._refine(self._lib.lsqr_refine_dense, params, max_rounds, labels_out)
        out.update(route=f["reserved"].copy())
        return out

    def assign_rigid(self, params, want_residuals=False, labels_out=None):
        """assign for absolute orientation (ls_type 0, or 2: weighted pairs), pivot calibration and ray intersection,
        which assign refuses (lsqr_assign_rigid): every record of the current upload / attach to the nearest of the
        models it agrees with.  params: M <= 64 rows of P parameters (7 / 6 / 3).  label = the smallest m that minimises
        residual(params[m], x) among the m with agree(params[m], x), -1 when none agrees and for a record with a
        non-finite slot (the weight included with ls_type 2); labels and residuals equal the first argmin over mask() /
        residuals() of the same rows bit for bit.  Any other model raises LsqrError(ERR_INVALID).  labels_out and the
        result as for assign."""
        return self._assign(self._lib.lsqr_assign_rigid, params, want_residuals, labels_out)

    def refine_rigid(self, params, max_rounds=8, labels_out=None):
        """refine for the models of assign_rigid (lsqr_refine_rigid): the same loop, and the refit of a model is its
        closed-form fit over its own records -- Horn's quaternion (weighted with ls_type 2), the pivot's normal
        equations, the rays' 3 x 3 system.  A model with fewer than K records, or whose solve gives no result (rays all
        parallel, frames all the same), keeps its row for that round.  The sums of a ray model are taken about the
        model's own point; those of an absolute orientation about the lowest-index record that is finite and agrees
        with the row as passed in, for the whole call.  Any other model raises LsqrError(ERR_INVALID).
        -> refine's dict."""
        return self._refine(self._lib.lsqr_refine_rigid, params, max_rounds, labels_out)[0]

    def _assign_grouped_args(self, groups, n_groups, params, n_models, labels_out):
        """the labels, rows and label buffer of assign_grouped / refine_grouped, groups and labels_out handled as in
        ransac_grouped_sequential -> (n, m, total, on_device, g, g_ptr, par, nm, labels, l_ptr); g keeps the host
        copy of the labels alive"""
        if self.cfg is None:
            raise L.LsqrError(L.ERR_STATE, "set_model has not been called")
        n = int(n_groups)
        if n < 0:
            raise ValueError("n_groups must not be negative")
        par = np.array(params, dtype=np.float64, order="C")  # a copy: refine_grouped writes it
        if par.ndim != 3 or par.shape[0] != n or par.shape[2] != self.P:
            raise ValueError("params must be shaped (n_groups, max_models, P)")
        m = par.shape[1]
        nm = np.full(n, m, dtype=np.uintp) if n_models is None else np.ascontiguousarray(n_models, dtype=np.uintp)
        if nm.shape != (n,):
            raise ValueError("one model count per group")
        total = int(self._lib.lsqr_count(self._h))
        on_device = hasattr(groups, "data_ptr")
        labels, l_ptr = None, None
        if on_device:
            if not groups.is_cuda or "int32" not in str(groups.dtype) or not groups.is_contiguous():
                raise ValueError("device groups must be a contiguous int32 device tensor")
            if groups.numel() != total:
                raise ValueError("one label per record")
            g, g_ptr = groups, groups.data_ptr()
            if labels_out is not None:
                t = labels_out
                if not (hasattr(t, "data_ptr") and t.is_cuda and "int32" in str(t.dtype) and t.is_contiguous()
                        and t.numel() == total):
                    raise ValueError("labels_out must be a contiguous int32 device tensor of one entry per record")
                labels, l_ptr = t, t.data_ptr()
        else:
            if labels_out is not None:
                raise ValueError("labels_out goes with device groups")
            g = np.asarray(groups)
            if g.dtype.kind not in "iu":
                raise ValueError("groups must be integers")
            if g.shape != (total,):
                raise ValueError("one label per record")
            # (labels beyond int32 are in no group, as -1 is)
            g = np.ascontiguousarray(np.where((g >= 0) & (g <= 0x7FFFFFFF), g, -1) if g.dtype != np.int32 else g,
                                     dtype=np.int32)
            g_ptr = L.ptr(g)
            labels = np.full(max(total, 1), -1, dtype=np.int32)
            l_ptr = L.ptr(labels)
        return n, m, total, on_device, g, g_ptr, par, nm, labels, l_ptr

    def assign_grouped(self, groups, n_groups, params, n_models=None, want_residuals=False, labels_out=None):
        """assign with one model set per label (lsqr_assign_grouped): group g is the records i with groups[i] == g, in
        upload order, and goes to the nearest of params[g, :n_models[g]] as assign decides it on those records alone,
        bit for bit.  params: (n_groups, max_models, P), max_models <= 64 -- what ransac_grouped_sequential returns as
        params, with its n_models; n_models defaults to max_models for every group.  A record in no group (a label
        that is negative or >= n_groups) or in a group without models gets -1 and +inf.
        groups / labels_out: a numpy integer array (host form), or contiguous int32 device tensors of one entry per
        record, as in ransac_grouped_sequential; the device form needs labels_out, allocates nothing on the device and
        leaves the residuals out (want_residuals must be False).
        -> dict: labels (the model index inside the record's group), residuals (None unless want_residuals), counts
        (uint64, (n_groups, max_models + 1): records per model, then the group's unassigned ones) and offsets (the
        prefix sums of the group sizes)."""
        return self._assign_grouped(self._lib.lsqr_assign_grouped, groups, n_groups, params, n_models, want_residuals,
                                    labels_out)

    def _assign_grouped(self, call, groups, n_groups, params, n_models, want_residuals, labels_out):
        """lsqr_assign_grouped or lsqr_assign_dense_grouped -> assign_grouped's dict"""
        n, m, total, on_device, g, g_ptr, par, nm, labels, l_ptr = self._assign_grouped_args(
            groups, n_groups, params, n_models, labels_out)
        if on_device and want_residuals:
            raise ValueError("want_residuals goes with host groups")
        if on_device and labels is None:
            raise ValueError("device groups need a device labels_out")
        res = np.full(max(total, 1), np.inf) if want_residuals else None
        counts = np.zeros((n, m + 1), dtype=np.uint64)
        offs = np.zeros(n + 1, dtype=np.uint64)
        self._chk(call(self._h, g_ptr, n, 1 if on_device else 0, L.ptr(par), L.ptr(nm), m, l_ptr, L.ptr(res),
                       L.ptr(counts), L.ptr(offs)))
        if not on_device:
            labels = labels[:total]
        return dict(labels=labels, residuals=res[:total] if res is not None else None, counts=counts, offsets=offs)

    def refine_grouped(self, groups, n_groups, params, n_models=None, max_rounds=8, labels_out=None):
        """refine with one model set per label (lsqr_refine_grouped): every group runs refine's loop on its own records
        and rows, bit for bit as refine runs it on those records alone, and stops on its own (converged, or at
        max_rounds); the records never leave the device.  Arguments as for assign_grouped; the device form may leave
        labels_out out.  The models of refine.
        -> dict: params ((n_groups, max_models, P); rows m >= n_models[g] as given), labels (None for the device form
        without labels_out), counts ((n_groups, max_models + 1)), status and n_used ((n_groups, max_models); status
        ERR_STATE where m >= n_models[g]), rounds (int64 per group), converged (bool per group) and offsets."""
        return self._refine_grouped(self._lib.lsqr_refine_grouped, groups, n_groups, params, n_models, max_rounds,
                                    labels_out)[0]

    def _refine_grouped(self, call, groups, n_groups, params, n_models, max_rounds, labels_out):
        """lsqr_refine_grouped, lsqr_refine_lm_grouped or lsqr_refine_dense_grouped -> (refine_grouped's dict, the fits
        as a structured array shaped (n_groups, max_models))"""
        n, m, total, on_device, g, g_ptr, par, nm, labels, l_ptr = self._assign_grouped_args(
            groups, n_groups, params, n_models, labels_out)
        if int(max_rounds) < 0:
            raise ValueError("max_rounds must not be negative")
        counts = np.zeros((n, m + 1), dtype=np.uint64)
        offs = np.zeros(n + 1, dtype=np.uint64)
        fits = (L.FitInfo * max(n * m, 1))()
        status = np.full(max(n * m, 1), L.ERR_STATE, dtype=np.int32)
        rounds = np.zeros(max(n, 1), dtype=np.uintp)
        conv = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(call(self._h, g_ptr, n, 1 if on_device else 0, L.ptr(par), L.ptr(nm), m, int(max_rounds), l_ptr,
                       L.ptr(counts), L.ptr(offs), fits, L.ptr(status), L.ptr(rounds), L.ptr(conv)))
        if labels is not None and not on_device:
            labels = labels[:total]
        f = np.ctypeslib.as_array(fits)[:n * m].reshape(n, m)
        return dict(params=par, labels=labels, counts=counts, status=status[:n * m].reshape(n, m),
                    n_used=f["n_used"].copy(), rounds=rounds[:n].astype(np.int64), converged=conv[:n].astype(bool),
                    offsets=offs), f

    def refine_lm_grouped(self, groups, n_groups, params, n_models=None, max_rounds=8, labels_out=None):
        """refine_grouped for the sphere with LS_GEOMETRIC, which refine_grouped refuses (lsqr_refine_lm_grouped): every
        group runs refine_lm's loop on its own records and rows, bit for bit as refine_lm runs it on those records
        alone -- the refit of a model is a Levenberg-Marquardt run from the algebraic fit of its records, all models
        of all groups still going evaluated together on the device.  A model whose run does not end with lm_info in
        1..4 (or that has fewer than K records, or no algebraic start) keeps the row it had before the round.
        Arguments as for refine_grouped.  Any other model raises LsqrError(ERR_INVALID).
        -> refine_grouped's dict, and per (group, model) for the group's last refit round lm_info, lm_nfev, cost and
        stall, each shaped (n_groups, max_models); zeros where no run started."""
        out, f = self._refine_grouped(self._lib.lsqr_refine_lm_grouped, groups, n_groups, params, n_models, max_rounds,
                                      labels_out)
        out.update(lm_info=f["lm_info"].copy(), lm_nfev=f["lm_nfev"].copy(), cost=f["cost"].copy(),
                   stall=f["reserved"].copy())
        return out

    def assign_dense_grouped(self, groups, n_groups, params, n_models=None, want_residuals=False, labels_out=None):
        """assign_grouped for the dense linear system, which assign_grouped refuses (lsqr_assign_dense_grouped): group
        g is the rows i with groups[i] == g, in upload order, and goes to the nearest of the regressions
        params[g, :n_models[g]] as assign_dense decides it on those rows alone, bit for bit.  params: (n_groups,
        max_models, n), max_models <= 64, n up to 64.  Arguments and result as for assign_grouped.  Any other model
        raises LsqrError(ERR_INVALID)."""
        return self._assign_grouped(self._lib.lsqr_assign_dense_grouped, groups, n_groups, params, n_models,
                                    want_residuals, labels_out)

    def refine_dense_grouped(self, groups, n_groups, params, n_models=None, max_rounds=8, labels_out=None):
        """refine_grouped for the dense linear system (lsqr_refine_dense_grouped): every group runs refine_dense's
        loop on its own rows and regressions, bit for bit as refine_dense runs it on those rows alone under the same
        options (dense_fast_solve, dense_dd), and stops on its own; the rows never leave the device.  Arguments as for
        refine_grouped.  Any other model raises LsqrError(ERR_INVALID).
        -> refine_grouped's dict, and route: per (group, model) the route of the group's last refit round (0: the
        elimination, 1: double-double from the group's rows, 2: dense_dd 0 and a pivot below 1e-6), shaped (n_groups,
        max_models); zeros where none ran."""
        out, f = self._refine_grouped(self._lib.lsqr_refine_dense_grouped, groups, n_groups, params, n_models,
                                      max_rounds, labels_out)
        out.update(route=f["reserved"].copy())
        return out

    def _many_records(self, problems):
        if self.cfg is None:
            raise L.LsqrError(L.ERR_STATE, "set_model has not been called")
        if isinstance(problems, tuple):
            recs, offs = problems
            recs = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, self.ND)
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
        else:
            parts = [np.asarray(a, dtype=np.float64).reshape(-1, self.ND) for a in problems]
            offs = np.zeros(len(parts) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([a.shape[0] for a in parts])
            recs = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, self.ND)))
        return recs, offs

    def _ransac_many(self, fn, problems, p, seeds, want_consensus, extra=()):
        """one call of fn (lsqr_ransac_many's signature) -> ransac_many's dict, with the fields `extra` of every
        problem's lsqr_fit_info after n_used"""
        recs, offs = self._many_records(problems)
        n = len(offs) - 1
        seeds = (1 + np.arange(n, dtype=np.uint64)) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if seeds.shape != (n,):
            raise ValueError("one seed per problem")
        params = np.zeros((max(n, 1), self.P))
        total = int(offs[-1]) if n else 0
        cons = np.zeros(max(total, 1), dtype=np.uint8) if want_consensus else None
        infos = (L.RansacInfo * max(n, 1))()
        status = np.zeros(max(n, 1), dtype=np.int32)
        # (p is None: the exhaustive search, which takes neither p nor seeds)
        draw = () if p is None else (float(p), L.ptr(seeds))
        self._chk(fn(self._h, L.ptr(recs), self.ND * 8, L.ptr(offs), n, *draw, L.ptr(params), L.ptr(cons), infos,
                     L.ptr(status)))
        status, params = status[:n], params[:n]
        params[status != L.OK] = 0.0
        inf = np.ctypeslib.as_array(infos)[:n]  # structured view of the lsqr_ransac_info array
        f = lambda name: inf[name].copy()
        fit = inf["fit"]
        return dict(status=status, fraction=f("fraction"), iterations=f("iterations"), best_index=f("best_index"),
                    best_votes=f("best_votes"), evaluated=f("evaluated"), n_params=f("n_params"),
                    n_used=fit["n_used"].copy(), **{k: fit[k].copy() for k in extra}, params=params,
                    consensus=cons[:total] if cons is not None else None, offsets=offs)

    def _fit_many(self, fn, problems, masks, keys, x0=None):
        """one call of fn (lsqr_dense_fit_many's signature; with x0, lsqr_lm_fit_many's) -> dict of status, params
        and the fields `keys` of every set's lsqr_fit_info"""
        recs, offs = self._many_records(problems)
        n = len(offs) - 1
        starts = ()
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, self.P)
            if x0.shape[0] != n:
                raise ValueError("one start per set")
            starts = (L.ptr(x0),)
        m = None
        if masks is not None:
            m = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
            if m.shape[0] != int(offs[-1]):
                raise ValueError("one mask byte per record")
        params = np.zeros((max(n, 1), self.P))
        fits = (L.FitInfo * max(n, 1))()
        status = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(fn(self._h, L.ptr(recs), self.ND * 8, L.ptr(offs), n, L.ptr(m), *starts, L.ptr(params), fits,
                     L.ptr(status)))
        status, params = status[:n], params[:n]
        params[status != L.OK] = 0.0
        fi = np.ctypeslib.as_array(fits)[:n]
        return dict(status=status, params=params, **{k: fi[k].copy() for k in keys})

    def ransac_many_lm(self, problems, p, seeds=None, want_consensus=True):
        """ransac_many with the geometric sphere's Levenberg-Marquardt finish (lsqr_ransac_many_lm); the context's
        model must be the sphere with ls_type LS_GEOMETRIC, else LsqrError(ERR_INVALID).  Problem j is decided as
        ransac(p, seed=seeds[j]) on its records alone.  -> ransac_many's dict plus the arrays lm_info, lm_nfev and
        cost of each problem's final fit."""
        return self._ransac_many(self._lib.lsqr_ransac_many_lm, problems, p, seeds, want_consensus,
                                 extra=("lm_info", "lm_nfev", "cost"))

    def ransac_many_exhaustive(self, problems, want_consensus=True):
        """Many independent problems of the exhaustive search (lsqr_ransac_many_exhaustive: every k-subset in
        lexicographic order, the first maximum wins; no p, no seeds) with the context's model: every model ransac_many
        takes, and the geometric sphere.  Problem j is decided as ransac_exhaustive() on its records alone; a problem
        of fewer than k records has status EMPTY.  -> ransac_many's dict (best_index: the winner's rank, see
        comb_unrank); with a geometric-sphere context also lm_info, lm_nfev and cost."""
        lm = self.cfg is not None and self.cfg.model == L.SPHERE and self.cfg.ls_type == L.LS_GEOMETRIC
        return self._ransac_many(self._lib.lsqr_ransac_many_exhaustive, problems, None, None, want_consensus,
                                 extra=("lm_info", "lm_nfev", "cost") if lm else ())

    def lm_fit_many(self, problems, x0, masks=None):
        """The geometric sphere fit (SphereParametersEstimator::geometricLeastSquaresEstimate) of many record sets
        in one call (lsqr_lm_fit_many).  problems as for ransac_many; x0: one start per set (n x P); masks
        (optional): one byte per record, aligned with the flat records.  -> dict of arrays: status (OK / EMPTY /
        ERR_INVALID for an empty set or mask), params (n x P, zero rows where status is not OK), lm_info, lm_nfev,
        cost and n_used."""
        return self._fit_many(self._lib.lsqr_lm_fit_many, problems, masks, ("lm_info", "lm_nfev", "cost", "n_used"),
                              x0=x0)

    def ransac_many_dense(self, problems, p, seeds=None, want_consensus=True):
        """ransac_many for the dense linear system (lsqr_ransac_many_dense, DenseLinearEquationSystemParameters-
        Estimator<double,n>); the context's model must be DENSE, else LsqrError(ERR_INVALID).  Records are n + 1
        doubles (a, b).  Problem j is decided as ransac(p, seed=seeds[j]) on its records alone.  -> ransac_many's
        dict plus the array reserved (fit.reserved: 1 where the finish took the double-double route)."""
        return self._ransac_many(self._lib.lsqr_ransac_many_dense, problems, p, seeds, want_consensus,
                                 extra=("reserved",))

    def dense_fit_many(self, problems, masks=None):
        """DenseLinearEquationSystemParametersEstimator::leastSquaresEstimate of many row sets in one call
        (lsqr_dense_fit_many).  problems as for ransac_many; masks (optional): one byte per record, aligned with the
        flat records.  -> dict of arrays: status (OK / EMPTY / ERR_INVALID for an empty set or mask), params (n x P,
        zero rows where status is not OK), n_params, reserved (1: the double-double route) and n_used."""
        return self._fit_many(self._lib.lsqr_dense_fit_many, problems, masks, ("n_params", "reserved", "n_used"))

    def batch_fit(self, seed, first, H, want_consensus=False):
        """One fixed-size batch end to end on the device (lsqr_batch_fit): winner of hypotheses
        [first, first + H) of the sampler stream, its consensus set, the final fit."""
        out = np.zeros(max(self.P, 32))
        cons = np.zeros(max(self.n, 1), dtype=np.uint8) if want_consensus else None
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_batch_fit(self._h, seed, first, H, L.ptr(out), L.ptr(cons),
                                                C.byref(info)), allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0),
                    consensus=cons[:self.n] if cons is not None else None, info=info)

    def batch_fit_enqueue(self, seed, first, H, slot=0):
        """chain a whole batch on the stream and return (lsqr_batch_fit_enqueue); closed-form fits only"""
        self._chk(self._lib.lsqr_batch_fit_enqueue(self._h, seed, first, H, slot))

    def batch_fit_wait(self, slot=0):
        """-> the dict of batch_fit() (without consensus) for the batch enqueued in `slot`"""
        out = np.zeros(max(self.P, 32))
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_batch_fit_wait(self._h, slot, L.ptr(out), C.byref(info)),
                       allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0), consensus=None,
                    info=info)

    def ransac_exhaustive(self, want_consensus=True):
        out = np.zeros(max(self.P, 32))
        cons = np.zeros(max(self.n, 1), dtype=np.uint8) if want_consensus else None
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_ransac_exhaustive(self._h, L.ptr(out), L.ptr(cons),
                                                        C.byref(info)), allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0),
                    consensus=cons[:self.n] if (cons is not None and info.best_votes > 0) else None,
                    info=info)

    def set_option(self, name, value):
        self._chk(self._lib.lsqr_set_option(self._h, name.encode(), int(value)))

    # ---- measurement --------------------------------------------------------------------
    def profile(self, on=True):
        self._chk(self._lib.lsqr_profile_enable(self._h, int(on)))
        self._chk(self._lib.lsqr_profile_reset(self._h))

    def profile_get(self, name):
        n = C.c_uint64(0)
        ms = C.c_double(0)
        self._chk(self._lib.lsqr_profile_get(self._h, L.KERNEL_IDS[name], C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def index_info(self):
        """-> dict(built, observations, cells, cell_points) of the spatial index (scan_index)"""
        out = (C.c_uint64 * 4)()
        self._chk(self._lib.lsqr_index_info(self._h, out))
        return {"built": bool(out[0]), "observations": int(out[1]), "cells": int(out[2]),
                "cell_points": int(out[3])}

    def scan_tiles_check(self):
        """the index's fp32 tiles against the sorted copy, every cell opened both ways on the device
        (lsqr_scan_tiles_check) -> dict(cell_points (0: no tiles), cells, words_differing, bytes)"""
        out = (C.c_uint64 * 4)()
        self._chk(self._lib.lsqr_scan_tiles_check(self._h, out))
        return {"cell_points": int(out[0]), "cells": int(out[1]), "words_differing": int(out[2]), "bytes": int(out[3])}

    def scan_workload(self, want_bounds=False):
        """level 1 of the two-level scan alone over the current batch (lsqr_scan_workload) ->
        dict(pairs, level1_evaluations, cells, cell_points[, bounds])"""
        H = self._lib.lsqr_num_hypotheses(self._h)
        ub = np.zeros(H, dtype=np.uint32) if want_bounds else None
        out = (C.c_uint64 * 8)()
        self._chk(self._lib.lsqr_scan_workload(self._h, L.ptr(ub), out))
        r = {"pairs": int(out[0]), "level1_evaluations": int(out[1]), "cells": int(out[2]),
             "cell_points": int(out[3]), "bounded": bool(out[4]), "pilots": int(out[5]),
             "second_pass": int(out[6]), "pairs_counted": int(out[7])}
        if want_bounds:
            r["bounds"] = ub
        return r

    def scan_work(self):
        """what the last scan of the current batch evaluated (lsqr_scan_work): models without a spatial index"""
        out = (C.c_uint64 * 8)()
        self._chk(self._lib.lsqr_scan_work(self._h, out))
        return {"early_exit": bool(out[0]), "row_hypothesis_pairs": int(out[1]), "row_hypothesis_pairs_all": int(out[2]),
                "candidates": int(out[3]), "dropped_first": int(out[4]), "alive_at_end": int(out[5]),
                "ambiguous_pairs": int(out[6]), "band_records": int(out[7])}

    def scan_pairs_counted(self):
        """the (hypothesis, cell) pairs the last counted two-level scan handed to its second level
        (lsqr_scan_pairs_counted) -> dict(pairs, masks, slab, table_entries)"""
        out = (C.c_uint64 * 4)()
        self._chk(self._lib.lsqr_scan_pairs_counted(self._h, out))
        return {"pairs": int(out[0]), "masks": bool(out[1]), "slab": bool(out[2]), "table_entries": int(out[3])}

    def synchronize(self):
        self._chk(self._lib.lsqr_synchronize(self._h))


class MultiContext:
    """Several devices from one process (lsqr_multi_*): the hypothesis stream sharded over one lsqr_ctx per entry
    of `devices`, exchanges by peer copies.  devices=[0, 0] puts two contexts on one GPU (tests)."""

    def __init__(self, devices):
        self._lib = L.load()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = self._lib.lsqr_multi_create(arr, len(devices), C.byref(h))
        if st != L.OK:
            raise L.LsqrError(st, "lsqr_multi_create(%s): %s" % (list(devices), self._lib.lsqr_status_string(st).decode()))
        self._h = h
        self.size = len(devices)
        self.cfg = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsqr_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st, allow_empty=False):
        if st == L.OK or (allow_empty and st == L.EMPTY):
            return st
        raise L.LsqrError(st, "%s (%s)" % (self._lib.lsqr_status_string(st).decode(),
                                           self._lib.lsqr_multi_last_error(self._h).decode()))

    def transport(self):
        """-> ("peer-copy" | "rccl", seconds spent bringing the RCCL communicators up)"""
        t = C.c_double(0.0)
        name = self._lib.lsqr_multi_transport(self._h, C.byref(t))
        return name.decode(), t.value

    def set_model(self, model, dim=3, delta=0.5, ls_type=L.LS_GEOMETRIC, aux=0.0):
        self.cfg = L.ModelCfg(int(model), int(dim), float(delta), int(ls_type), 0, float(aux))
        self._chk(self._lib.lsqr_multi_set_model(self._h, C.byref(self.cfg)))
        self.P = self._lib.lsqr_num_params(C.byref(self.cfg))
        return self

    def upload(self, data):
        a = np.ascontiguousarray(data, dtype=np.float64)
        a = a.reshape(-1, a.shape[-1])
        self._chk(self._lib.lsqr_multi_upload(self._h, L.ptr(a), a.shape[0], a.shape[1] * 8))
        self.n = a.shape[0]
        return self

    def set_option(self, name, value):
        for r in range(self.size):
            c = self._lib.lsqr_multi_ctx(self._h, r)
            st = self._lib.lsqr_set_option(C.c_void_p(c), name.encode(), int(value))
            if st != L.OK:
                raise L.LsqrError(st, "lsqr_set_option(%s)" % name)

    def batch_fit(self, seed, first, H, want_consensus=False):
        out = np.zeros(max(self.P, 64))
        cons = np.zeros(max(self.n, 1), dtype=np.uint8) if want_consensus else None
        info = L.RansacInfo()
        st = self._chk(self._lib.lsqr_multi_batch_fit(self._h, seed, first, H, L.ptr(out), L.ptr(cons),
                                                      C.byref(info)), allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0),
                    consensus=cons[:self.n] if cons is not None else None, info=info)

    def ransac(self, p, seed=1, want_consensus=True):
        out = np.zeros(max(self.P, 64))
        cons = np.zeros(max(self.n, 1), dtype=np.uint8) if want_consensus else None
        info = L.RansacInfo()
        st = self._lib.lsqr_multi_ransac(self._h, float(p), seed, L.ptr(out), L.ptr(cons), C.byref(info))
        if st == L.ERR_INVALID and info.iterations == 0:
            return dict(status=st, fraction=0.0, params=None, consensus=None, info=info)
        self._chk(st, allow_empty=True)
        return dict(status=st, fraction=info.fraction,
                    params=out[:info.n_params].copy() if st == L.OK else np.zeros(0),
                    consensus=cons[:self.n] if (cons is not None and info.best_votes > 0) else None, info=info)


def replay(n, k, p, subsets, valid, votes, dedup=True):
    """Host replay of RANSAC.hxx:49-117 over one batch (exposed for tests)."""
    lib = L.load()
    st = (C.c_uint64 * 6)()
    lib.lsqr_replay_init(n, k, p, st)
    s = np.ascontiguousarray(subsets, dtype=np.uint32)
    v = np.ascontiguousarray(valid, dtype=np.uint8)
    c = np.ascontiguousarray(votes, dtype=np.uint32)
    d = lib.lsqr_dedup_create(k) if dedup else None
    used = lib.lsqr_replay(n, k, p, L.ptr(s), L.ptr(v), L.ptr(c), len(c), 0, d, st)
    if d:
        lib.lsqr_dedup_destroy(d)
    return dict(used=used, i=st[0], num_tries=st[1], best_votes=st[2], best_index=st[3],
                has_best=bool(st[4]), done=bool(st[5]))


def comb_count(n, k):
    """C(n, k) as the exhaustive search counts its hypotheses (lsqr_comb_count; host only); LsqrError(ERR_INVALID)
    when k is outside 1..64 or the value does not fit in 64 bits."""
    out = C.c_uint64(0)
    st = L.load().lsqr_comb_count(int(n), int(k), C.byref(out))
    if st != L.OK:
        raise L.LsqrError(st, "C(%d, %d) is not representable" % (n, k))
    return out.value


def comb_unrank(n, k, rank):
    """The rank-th k-subset of range(n) in the exhaustive search's order (lsqr_comb_unrank; host only): the subset
    behind a best_index of ransac_exhaustive / ransac_many_exhaustive, as a uint32 array of increasing indices."""
    out = np.zeros(max(int(k), 1), dtype=np.uint32)
    st = L.load().lsqr_comb_unrank(int(n), int(k), int(rank), L.ptr(out))
    if st != L.OK:
        raise L.LsqrError(st, "no subset of rank %d among C(%d, %d)" % (rank, n, k))
    return out
