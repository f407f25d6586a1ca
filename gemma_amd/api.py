"""Host-side mirror of the GEMMA interfaces on the kinship + univariate-LMM path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (file:line relative to the
GEMMA tree) so that the parity tests read like the reference's own tests:

    fast_dgemm            src/fastblas.h:34-36
    CenterMatrix          src/mathfunc.cpp:147-177
    EigenDecomp_Zeroed    src/lapack.cpp:260-291
    CalcUtX               src/mathfunc.cpp:504-506
    CalcKin / BimbamKin / PlinkKin   src/param.cpp:1300-1321, src/gemma_io.cpp:1418-1738
    CalcLambdaNull / CalcPve         src/lmm.cpp:2143-2205
    CalcLambdaNullPanel              the same for every column of U^T Y at once, with CalcLmmVgVeBeta's beta :2210-2281
    class LMM  (CopyFromParam fields, Analyze*, WriteFiles)   src/lmm.h:49-125

Arrays may be numpy arrays (host entry points; the library stages through HBM) or torch CUDA
tensors (device entry points on torch's current stream: torch is only the allocator/stream here).
All compute happens in gemma_amd/libgemma_hip.so; nothing in this module has a CPU fallback.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L

SUMSTAT_DTYPE = np.dtype([(k, "f8") for k in
                          ("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score",
                           "logl_H1")])
SCORE_DTYPE = np.dtype([(k, "f8") for k in ("beta", "se", "p_score")])  # gemma_score_rec
SCORE_HIT_DTYPE = np.dtype([("snp", "u4"), ("pheno", "u4"), ("beta", "f8"), ("se", "f8"), ("p_score", "f8")])  # gemma_score_hit
SCORE_BEST_DTYPE = np.dtype([("beta", "f8"), ("se", "f8"), ("p_score", "f8"), ("snp", "i8")])  # gemma_score_best
NULL_DTYPE = np.dtype([(k, "f8") for k in ("l_mle_null", "logl_mle_H0", "l_remle_null", "logl_remle_H0", "pve", "pve_se", "vg_remle",
                                             "ve_remle")])  # gemma_null_fit
_MVPAIR_BLOCK = [("Vg", "f8", 3), ("Ve", "f8", 3), ("VVg", "f8", 3), ("VVe", "f8", 3)] + \
    [(k, "f8") for k in ("rg", "var_rg", "re", "var_re", "logl")]
MVPAIR_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("status", "i4"), ("pad", "i4"), ("remle", _MVPAIR_BLOCK),
                         ("mle", _MVPAIR_BLOCK)])  # gemma_mvpair_fit
LMM_BATCH_SIZE = 20000  # src/lmm.h:33
K_BATCH_SIZE = 20000  # src/param.h:32


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _np64(a, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64:
        raise TypeError("%s must be a float64 numpy array" % name)
    if a.ndim == 2 and a.size and a.strides[1] != 8:  # (numpy gives an empty array strides of 0: K == 0 is C = beta C)
        raise ValueError("%s must be row-major with unit column stride" % name)
    return a


def _ld(a):
    return a.shape[1] if a.ndim == 2 and a.shape[0] <= 1 else (a.strides[0] // 8 if a.ndim == 2 else a.shape[0])


def _row_ld(a):
    """Row stride of a 2-D genotype block in items.  numpy is free to report any stride for an axis of length 1, so a block of
    one SNP takes its width (with one row every stride >= the width is the same layout)."""
    return a.shape[1] if a.shape[0] <= 1 else a.strides[0] // a.itemsize


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tld(t):
    if t.dim() != 2 or (t.numel() and t.stride(1) != 1):  # (an empty tensor's strides may be 0)
        raise ValueError("device matrices must be 2-D row-major")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _block_dims(geno, geno_kind, l=None, ld=None):
    """(l, ld) of a genotype block, numpy or torch: l SNPs -- the columns of individual-major input (the reference's Xlarge), the rows
    otherwise -- and the row stride in items.  Values the caller gives are kept."""
    if l is None:
        l = geno.shape[1] if geno_kind == L.GENO_F64_IDV_MAJOR else geno.shape[0]
    if ld is None:
        ld = _tld(geno) if _is_torch(geno) else _row_ld(geno)
    return l, ld


def _scan(setup, set_indicator, finish, indicator_idv, geno, batch, block, prepare=None):
    """The frame of every Analyze*: setup(), the indicator, prepare() (what else the state needs before its first block), then
    block(s0, geno[s0:s0 + batch]) for every block -> the list of their results.  finish() runs whatever a block raises."""
    setup()
    try:
        if indicator_idv is not None:
            set_indicator(indicator_idv)
        if prepare is not None:
            prepare()
        return [block(s0, geno[s0:s0 + batch]) for s0 in range(0, geno.shape[0], batch)]
    finally:
        finish()


def init(device=-1, verbose=0):
    L.check(L.lib().gemma_hip_init(device, verbose), "gemma_hip_init")


def device_info():
    name = C.create_string_buffer(256)
    cu = C.c_int()
    mem = C.c_size_t()
    L.check(L.lib().gemma_hip_device_info(name, 256, C.byref(cu), C.byref(mem)), "device_info")
    return name.value.decode(), cu.value, mem.value


def profile_enable(on=True):
    L.check(L.lib().gemma_hip_profile_enable(1 if on else 0), "profile_enable")


def profile_read(stage, reset=False):
    ms = C.c_double()
    n = C.c_long()
    L.check(L.lib().gemma_hip_profile_read(stage, C.byref(ms), C.byref(n), 1 if reset else 0), "profile_read")
    return ms.value, n.value


UTX_PATHS = {0: "fp64 MFMA GEMM", 1: "int8 digits, hard calls", 2: "int8 digits, dosages k/100", 3: "int8 digits, dosages k/1000"}


def last_utx_path():
    """What the last U^T x (LMM.batch, LMM.dbg_utx) ran on: a key of UTX_PATHS."""
    p = C.c_int()
    L.check(L.lib().gemma_hip_dbg_last_utx_path(C.byref(p)), "dbg_last_utx_path")
    return p.value


def last_utx_kernel():
    """The matrix kernel the last U^T x launched (gemma_hip_dbg_last_utx_kernel): dict(variant, rows, digits, fuse, raster,
    launches, name) -- name is the kernel symbol as rocprofv3 prints it."""
    k = L.UtxKernelInfo()
    L.check(L.lib().gemma_hip_dbg_last_utx_kernel(C.byref(k)), "dbg_last_utx_kernel")
    return {"variant": k.variant, "rows": k.rows, "digits": k.digits, "fuse": k.fuse, "raster": k.raster,
            "launches": k.launches, "name": k.name.decode()}


def last_mvlmm_kernel(which):
    """(form, d, rows) of the last multivariate per-SNP launch (which = 0) / null fit (1): form is L.MV_KERNEL_FIXED or _RUN_TIME."""
    f, d, r = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().gemma_hip_dbg_last_mvlmm_kernel(which, C.byref(f), C.byref(d), C.byref(r)), "dbg_last_mvlmm_kernel")
    return f.value, d.value, r.value


def last_block_missing():
    """gemma_hip_dbg_last_block_missing: 1 / 0 = the last records product's block held / did not hold a missing call (a block without
    one takes the genotype product alone); -1 = the complete-block form is off or no such product ran."""
    a = C.c_int()
    L.check(L.lib().gemma_hip_dbg_last_block_missing(C.byref(a)), "dbg_last_block_missing")
    return a.value


def reload_env():
    """Have the library re-read its GEMMA_HIP_* switches (it reads them once per setup, never per launch)."""
    L.check(L.lib().gemma_hip_reload_env(), "reload_env")


# ----------------------------------------------------------------------------- B2
def fast_dgemm(TransA, TransB, alpha, A, B, beta, Cm):
    """C = alpha*op(A)*op(B) + beta*C (row-major).  Shape mismatch -> GemmaHipError(EINVAL), the
    reference's fail_msg("Range error in dgemm") (src/fastblas.cpp:207)."""
    ta, tb = TransA.upper()[0], TransB.upper()[0]
    M, N = Cm.shape
    if ta not in "NT" or tb not in "NT":
        raise L.GemmaHipError(L.EINVAL, "fast_dgemm", "bad transpose flag")
    Ka = A.shape[0] if ta == "T" else A.shape[1]
    Ma = A.shape[1] if ta == "T" else A.shape[0]
    Kb = B.shape[1] if tb == "T" else B.shape[0]
    Nb = B.shape[0] if tb == "T" else B.shape[1]
    if Ma != M or Nb != N or Ka != Kb:
        raise L.GemmaHipError(L.EINVAL, "fast_dgemm", "Range error in dgemm")
    if _is_torch(Cm):
        rc = L.lib().gemma_hip_dgemm_d(ta.encode(), tb.encode(), M, N, Ka, alpha, C.c_void_p(A.data_ptr()),
                                       _tld(A), C.c_void_p(B.data_ptr()), _tld(B), beta,
                                       C.c_void_p(Cm.data_ptr()), _tld(Cm), _stream())
    else:
        _np64(A, "A"); _np64(B, "B"); _np64(Cm, "C")
        rc = L.lib().gemma_hip_dgemm(ta.encode(), tb.encode(), M, N, Ka, alpha, _ptr(A), _ld(A), _ptr(B),
                                     _ld(B), beta, _ptr(Cm), _ld(Cm))
    L.check(rc, "fast_dgemm")
    return Cm


fast_eigen_dgemm = fast_dgemm  # src/fastblas.h:37-39 (historical alias)


# ----------------------------------------------------------------------------- B3
def CenterMatrix(G):
    """In place, src/mathfunc.cpp:147-177."""
    n = G.shape[0]
    if _is_torch(G):
        L.check(L.lib().gemma_hip_center_d(C.c_void_p(G.data_ptr()), n, _stream()), "CenterMatrix")
    else:
        _np64(G, "G")
        if not G.flags.c_contiguous:
            raise ValueError("G must be contiguous")
        L.check(L.lib().gemma_hip_center(_ptr(G), n), "CenterMatrix")
    return G


def EigenDecomp_Zeroed(G, U, eval_):
    """G is destroyed; U gets eigenvectors in columns, eval_ ascending with values < 1e-10 zeroed.
    Returns trace_G = mean(eval) (src/lapack.cpp:260-291)."""
    n = G.shape[0]
    tr = C.c_double()
    if _is_torch(G):
        rc = L.lib().gemma_hip_eigh_d(C.c_void_p(G.data_ptr()), n, C.c_void_p(U.data_ptr()),
                                      C.c_void_p(eval_.data_ptr()), C.byref(tr), _stream())
    else:
        _np64(G, "G"); _np64(U, "U"); _np64(eval_, "eval")
        rc = L.lib().gemma_hip_eigh(_ptr(G), n, _ptr(U), _ptr(eval_), C.byref(tr))
    L.check(rc, "EigenDecomp_Zeroed")
    return tr.value


def eigh_reserve(n):
    """gemma_hip_eigh_reserve: allocate the eigensolver's workspace of order n ahead of the solve and keep the buffers of every later
    solve in the library's pool (csrc/eigh.hip.h, EigPool) until eigh_release()."""
    L.check(L.lib().gemma_hip_eigh_reserve(int(n)), "eigh_reserve")


def eigh_release():
    """gemma_hip_eigh_release: hand the pool's idle buffers back; returns the bytes freed."""
    b = C.c_size_t()
    L.check(L.lib().gemma_hip_eigh_release(C.byref(b)), "eigh_release")
    return b.value


def EigenDecomp_Zeroed_sharded(G, U, eval_):
    """EigenDecomp_Zeroed as a COLLECTIVE over the library's communicator (gemma_amd.dist.native_comm_init): every rank passes
    the same device matrix G (destroyed) and receives the same (U, eval_); the two back-transformations are shared out by
    eigenvector.  torch tensors on the device only."""
    n = G.shape[0]
    tr = C.c_double()
    rc = L.lib().gemma_hip_eigh_sharded_d(C.c_void_p(G.data_ptr()), n, C.c_void_p(U.data_ptr()),
                                          C.c_void_p(eval_.data_ptr()), C.byref(tr), _stream())
    L.check(rc, "EigenDecomp_Zeroed_sharded")
    return tr.value


def CalcUtX(U, X):
    """UtX = U^T X (src/mathfunc.cpp:504-506).  X: n x m (or n,) numpy."""
    X2 = np.ascontiguousarray(X.reshape(X.shape[0], -1), dtype=np.float64)
    n, m = X2.shape
    out = np.zeros((n, m))
    L.check(L.lib().gemma_hip_calc_utx(_ptr(_np64(U, "U")), _ptr(X2), n, m, _ptr(out)), "CalcUtX")
    return out.reshape(X.shape)


# ----------------------------------------------------------------------------- B1
def kin_begin(n_total, k_mode=1):
    L.check(L.lib().gemma_hip_kin_begin(n_total, k_mode), "kin_begin")


def kin_add(geno, geno_kind, l=None, ld=None):
    l, ld = _block_dims(geno, geno_kind, l, ld)
    if _is_torch(geno):
        rc = L.lib().gemma_hip_kin_add_d(geno_kind, C.c_void_p(geno.data_ptr()), l, ld, _stream())
    else:
        rc = L.lib().gemma_hip_kin_add(geno_kind, _ptr(geno), l, ld)
    L.check(rc, "kin_add")


def kin_end(K=None):
    ns = C.c_size_t()
    if K is not None and _is_torch(K):
        L.check(L.lib().gemma_hip_kin_end_d(C.c_void_p(K.data_ptr()), C.byref(ns), _stream()), "kin_end")
    else:
        L.check(L.lib().gemma_hip_kin_end(_ptr(K) if K is not None else None, C.byref(ns)), "kin_end")
    return ns.value


# ---- the device-resident chain (include/gemma_hip.h "kept"): K, U, eval never leave the device; with a communicator of several
# ranks kin_end_keep(allreduce=True) is the ONE ncclAllReduce of the SNP-sharded kinship and EigenDecomp_kept_K(sharded=True) the
# collective decomposition -- the flow of tests/cpp/gemma_file_driver.cpp -gpus N and of bench.py --gpus N
def kin_end_keep(allreduce=False):
    """Ends kin_begin / kin_add and KEEPS K on the device; allreduce: sum the ranks' partial kinships first (every rank then holds
    the kinship of all SNPs).  Returns the SNP count (of all ranks with allreduce)."""
    ns = C.c_size_t()
    L.check(L.lib().gemma_hip_kin_end_keep(C.byref(ns), 1 if allreduce else 0), "kin_end_keep")
    return ns.value


def EigenDecomp_kept_K(ni_total, indicator_idv=None, sharded=False):
    """Sub-select (ReadFile_kin's indicator), CenterMatrix, EigenDecomp_Zeroed of the kept K, all on the device; U and eval stay
    there (lmm setup_kept / CalcUtX_kept use them).  sharded: the collective form (every rank holds the same kept K).  Returns
    (eval numpy, trace_G)."""
    ind = None if indicator_idv is None else np.ascontiguousarray(indicator_idv, dtype=np.int32)
    n = int(ni_total if ind is None else int((ind != 0).sum()))
    ev = np.zeros(n)
    tr = C.c_double()
    fn = L.lib().gemma_hip_eigh_kept_K_sharded if sharded else L.lib().gemma_hip_eigh_kept_K
    L.check(fn(_ptr(ind) if ind is not None else None, ni_total, _ptr(ev), C.byref(tr)), "EigenDecomp_kept_K")
    return ev, tr.value


def CalcUtX_kept(X):
    """U^T X on the kept U (host X: n x m or n,; returns numpy of the same shape)."""
    X2 = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(len(X), -1))
    out = np.zeros_like(X2)
    L.check(L.lib().gemma_hip_calc_utx_kept(_ptr(X2), X2.shape[0], X2.shape[1], _ptr(out)), "CalcUtX_kept")
    return out.reshape(np.asarray(X).shape)


def kept_release():
    L.check(L.lib().gemma_hip_kept_release(), "kept_release")


def comm_info():
    """(rank, world, transport) of the library's communicator: transport 0 none, 1 RCCL, 2 the shm test transport."""
    r, w, t = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().gemma_hip_comm_info(C.byref(r), C.byref(w), C.byref(t)), "comm_info")
    return r.value, w.value, t.value


def comm_stats():
    """gemma_hip_comm_stats as a dict: calls, 1-GiB pieces and bytes per collective since comm_init (seconds only with
    GEMMA_HIP_COMM_TIMING=1 in the environment)."""
    st = L.CommStats()
    L.check(L.lib().gemma_hip_comm_stats(C.byref(st)), "comm_stats")
    return {k: getattr(st, k) for k, _ in L.CommStats._fields_}


def CalcKin(geno, geno_kind, n_total, k_mode=1, batch=K_BATCH_SIZE):
    """PARAM::CalcKin -> BimbamKin / PlinkKin: streams `geno` (SNP-major rows) in blocks of
    K_BATCH_SIZE SNPs and returns the n_total x n_total kinship matrix (numpy)."""
    kin_begin(n_total, k_mode)
    p = geno.shape[0]
    for s0 in range(0, p, batch):
        kin_add(geno[s0:s0 + batch], geno_kind)
    K = np.zeros((n_total, n_total))
    kin_end(K)
    return K


def SnpQC(geno, geno_kind, indicator_idv, W, maf_level=0.01, miss_level=0.05, hwe_level=0.0, r2_level=0.9999):
    """First-pass SNP filters of ReadFile_geno / ReadFile_bed (src/gemma_io.cpp:639-873 / :876-1064) on device.
    geno: SNP-major rows over ALL individuals (fp64 with NaN, or .bed bytes); W: covariates of the analysed
    individuals.  Returns (indicator_snp, maf, n_miss)."""
    ind = None if indicator_idv is None else np.ascontiguousarray(indicator_idv, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64).reshape(len(W), -1)
    n, c = W.shape
    l = geno.shape[0]
    ni_total = n if ind is None else ind.size
    cfg = L.QcCfg(maf_level, miss_level, hwe_level, r2_level)
    out_i = np.zeros(l, dtype=np.int32)
    out_maf = np.zeros(l)
    out_nm = np.zeros(l, dtype=np.uint64)
    L.check(L.lib().gemma_hip_snp_qc(geno_kind, _ptr(geno), l, _row_ld(geno),
                                     _ptr(ind) if ind is not None else None, ni_total, _ptr(W), n, c, C.byref(cfg),
                                     _ptr(out_i), _ptr(out_maf), _ptr(out_nm)), "SnpQC")
    return out_i, out_maf, out_nm.astype(np.int64)


def CalcKinLOCO(geno, geno_kind, n_total, chr_of_snp, k_mode=1, batch=K_BATCH_SIZE):
    """-loco for every chromosome at once (torch device tensors inside): the all-SNP kinship plus one
    per-chromosome kinship, combined on device as (ns K - ns_c K_c)/(ns - ns_c).  Returns {chr: K_loco numpy}."""
    import torch
    chr_of_snp = np.asarray(chr_of_snp)
    dev = torch.device("cuda", torch.cuda.current_device())
    Kall = torch.empty((n_total, n_total), dtype=torch.float64, device=dev)
    kin_begin(n_total, k_mode)
    for s0 in range(0, geno.shape[0], batch):
        kin_add(geno[s0:s0 + batch], geno_kind)
    ns_all = kin_end(Kall)
    out = {}
    for ch in sorted(set(chr_of_snp.tolist())):
        sel = np.flatnonzero(chr_of_snp == ch)
        Kc = torch.empty_like(Kall)
        kin_begin(n_total, k_mode)
        g = np.ascontiguousarray(geno[sel])
        for s0 in range(0, g.shape[0], batch):
            kin_add(g[s0:s0 + batch], geno_kind)
        ns_c = kin_end(Kc)
        L.check(L.lib().gemma_hip_kin_loco_d(C.c_void_p(Kall.data_ptr()), ns_all, C.c_void_p(Kc.data_ptr()), ns_c,
                                             n_total, _stream()), "CalcKinLOCO")
        torch.cuda.synchronize()
        out[ch] = Kc.cpu().numpy()
    return out


def WriteMatrix10(M):
    """The text hand-off `-gk` -> `-lmm`: PARAM::WriteMatrix at precision(10) (src/param.cpp:1886-1911) read back
    by ReadFile_kin (src/gemma_io.cpp:1186-1243).  Returns the matrix as the second GEMMA run would see it."""
    flat = np.array([float("%.10g" % v) for v in np.asarray(M, dtype=np.float64).ravel()])
    return flat.reshape(np.asarray(M).shape)


# ----------------------------------------------------------------------------- null model
def CalcLambdaNull(eval_, UtW, Uty, l_min=1e-5, l_max=1e5, n_region=10, trace_G=1.0):
    """Returns dict(l_mle_null, logl_mle_H0, l_remle_null, logl_remle_H0, pve, pve_se, vg, ve):
    src/gemma.cpp:2711-2750."""
    UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(len(eval_), -1)
    out = np.zeros(8)
    n, c = UtW.shape
    # converted copies stay bound to names until the call returns (_ptr keeps only the address)
    ev_c = _np64(np.ascontiguousarray(eval_, dtype=np.float64), "eval")
    Uty_c = np.ascontiguousarray(Uty, dtype=np.float64)
    L.check(L.lib().gemma_hip_lmm_null(n, c, _ptr(ev_c), _ptr(UtW), _ptr(Uty_c), l_min, l_max,
                                       n_region, trace_G, _ptr(out)), "CalcLambdaNull")
    keys = ("l_mle_null", "logl_mle_H0", "l_remle_null", "logl_remle_H0", "pve", "pve_se", "vg_remle",
            "ve_remle")
    return dict(zip(keys, out.tolist()))


def CalcLambdaNullPanel(eval_, UtW, UtY, l_min=1e-5, l_max=1e5, n_region=10, trace_G=1.0, want_beta=False):
    """CalcLambdaNull for every column of UtY (n x T) in one launch per chunk of columns, one wavefront per phenotype: row t holds,
    bit for bit, what CalcLambdaNull gives for UtY[:, t].  numpy in: a (T,) NULL_DTYPE array; torch device tensors in: a (T, 8)
    device tensor in the field order of NULL_DTYPE.  want_beta: also the (T, c) covariate effects at l_remle_null and their
    standard errors (CalcLmmVgVeBeta, src/lmm.cpp:2210-2281; c <= 16), NaN in the row of a phenotype whose UtW' H UtW is not
    positive definite."""
    if _is_torch(UtY):
        import torch
        for name, t in (("eval", eval_), ("UtW", UtW), ("UtY", UtY)):
            if not _is_torch(t) or t.dtype != torch.float64 or not t.is_cuda:
                raise TypeError("CalcLambdaNullPanel: %s must be a float64 device tensor" % name)
        n = UtY.shape[0]
        if UtY.dim() == 1:
            UtY = UtY.reshape(n, 1)
        if UtW.dim() == 1:
            UtW = UtW.reshape(-1, 1)
        UtW, UtY, eval_ = UtW.contiguous(), UtY.contiguous(), eval_.contiguous()
        _tld(UtW), _tld(UtY)  # 2-D row-major
        if eval_.dim() != 1 or eval_.shape[0] != n or UtW.shape[0] != n:
            raise ValueError("CalcLambdaNullPanel: eval (%d), UtW (%d rows) and UtY (%d rows) disagree"
                             % (eval_.shape[0], UtW.shape[0], n))
        T, c = UtY.shape[1], UtW.shape[1]
        fit = torch.empty((T, 8), dtype=torch.float64, device=UtY.device)
        beta = torch.empty((T, c), dtype=torch.float64, device=UtY.device) if want_beta else None
        se = torch.empty((T, c), dtype=torch.float64, device=UtY.device) if want_beta else None
        L.check(L.lib().gemma_hip_lmm_null_panel_d(n, c, T, C.c_void_p(eval_.data_ptr()), C.c_void_p(UtW.data_ptr()),
                                                   C.c_void_p(UtY.data_ptr()), l_min, l_max, n_region, trace_G,
                                                   C.c_void_p(fit.data_ptr()), C.c_void_p(beta.data_ptr()) if want_beta else None,
                                                   C.c_void_p(se.data_ptr()) if want_beta else None, _stream()),
                "CalcLambdaNullPanel")
        return (fit, beta, se) if want_beta else fit
    n = len(eval_)
    UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
    UtY_c = np.ascontiguousarray(UtY, dtype=np.float64).reshape(n, -1)
    ev_c = _np64(np.ascontiguousarray(eval_, dtype=np.float64), "eval")
    c, T = UtW.shape[1], UtY_c.shape[1]
    if ev_c.ndim != 1 or UtW.shape[0] != n or UtY_c.shape[0] != n:
        raise ValueError("CalcLambdaNullPanel: eval (%d), UtW and UtY disagree in their rows" % n)
    fit = np.zeros(T, dtype=NULL_DTYPE)
    beta = np.zeros((T, c)) if want_beta else None
    se = np.zeros((T, c)) if want_beta else None
    L.check(L.lib().gemma_hip_lmm_null_panel(n, c, T, _ptr(ev_c), _ptr(UtW), _ptr(UtY_c), l_min, l_max, n_region, trace_G,
                                             _ptr(fit), _ptr(beta) if want_beta else None, _ptr(se) if want_beta else None),
            "CalcLambdaNullPanel")
    return (fit, beta, se) if want_beta else fit


def CalcMvNullPairs(eval_, UtW, UtY, pairs=None, opt=None, want_beta=False, l_min=1e-5, l_max=1e5, n_region=10):
    """The two-trait null fit of every listed pair of columns of UtY (n x T), one wavefront per pair: per pair what
    MVLMM.fit_null gives on the two columns (Vg, Ve, logl, B in the same bits), the variances VVg / VVe behind se(Vg) / se(Ve), and
    the genetic / residual correlations with their delta-method variances.  pairs: (m, 2) ints with i < j, or None for all i < j row
    by row.  opt: an L.MvOpt (None: the PARAM defaults).  numpy in: a (m,) MVPAIR_DTYPE array; torch device tensors in: a (m, 36)
    float64 device tensor whose rows are the same records (view them with .cpu().numpy().view(MVPAIR_DTYPE)).  want_beta: also B and
    VB, (m, 2, 2, c): pass (REMLE, MLE), trait, covariate."""
    popt = C.byref(opt) if opt is not None else None
    if _is_torch(UtY):
        import torch
        for name, t in (("eval", eval_), ("UtW", UtW), ("UtY", UtY)):
            if not _is_torch(t) or t.dtype != torch.float64 or not t.is_cuda:
                raise TypeError("CalcMvNullPairs: %s must be a float64 device tensor" % name)
        n = UtY.shape[0]
        if UtW.dim() == 1:
            UtW = UtW.reshape(-1, 1)
        UtW, UtY, eval_ = UtW.contiguous(), UtY.contiguous(), eval_.contiguous()
        _tld(UtW), _tld(UtY)  # 2-D row-major
        if eval_.dim() != 1 or eval_.shape[0] != n or UtW.shape[0] != n:
            raise ValueError("CalcMvNullPairs: eval (%d), UtW (%d rows) and UtY (%d rows) disagree" % (eval_.shape[0], UtW.shape[0], n))
        T, c = UtY.shape[1], UtW.shape[1]
        if pairs is not None:
            pairs = torch.as_tensor(pairs, dtype=torch.int32, device=UtY.device).reshape(-1, 2).contiguous()
        m = T * (T - 1) // 2 if pairs is None else pairs.shape[0]
        fit = torch.empty((m, MVPAIR_DTYPE.itemsize // 8), dtype=torch.float64, device=UtY.device)
        B = torch.empty((m, 2, 2, c), dtype=torch.float64, device=UtY.device) if want_beta else None
        VB = torch.empty((m, 2, 2, c), dtype=torch.float64, device=UtY.device) if want_beta else None
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        L.check(L.lib().gemma_hip_mvlmm_null_pairs_d(n, c, T, vp(eval_), vp(UtW), vp(UtY), vp(pairs), 0 if pairs is None else m,
                                                     l_min, l_max, n_region, popt, vp(fit), vp(B), vp(VB), _stream()),
                "CalcMvNullPairs")
        return (fit, B, VB) if want_beta else fit
    n = len(eval_)
    UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
    UtY_c = np.ascontiguousarray(UtY, dtype=np.float64).reshape(n, -1)
    ev_c = _np64(np.ascontiguousarray(eval_, dtype=np.float64), "eval")
    c, T = UtW.shape[1], UtY_c.shape[1]
    if ev_c.ndim != 1 or UtW.shape[0] != n or UtY_c.shape[0] != n:
        raise ValueError("CalcMvNullPairs: eval (%d), UtW and UtY disagree in their rows" % n)
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    m = T * (T - 1) // 2 if pairs is None else pairs.shape[0]
    fit = np.zeros(m, dtype=MVPAIR_DTYPE)
    B = np.zeros((m, 2, 2, c)) if want_beta else None
    VB = np.zeros((m, 2, 2, c)) if want_beta else None
    L.check(L.lib().gemma_hip_mvlmm_null_pairs(n, c, T, _ptr(ev_c), _ptr(UtW), _ptr(UtY_c),
                                               pairs.ctypes.data_as(C.POINTER(C.c_int)) if pairs is not None else None,
                                               0 if pairs is None else m, l_min, l_max, n_region, popt,
                                               fit.ctypes.data_as(C.POINTER(L.MvPairFit)), _ptr(B) if want_beta else None,
                                               _ptr(VB) if want_beta else None), "CalcMvNullPairs")
    return (fit, B, VB) if want_beta else fit


def mv_pair_matrices(fit, T, block="remle"):
    """A CalcMvNullPairs result (MVPAIR_DTYPE) -> the T x T matrices rg, re and their standard errors se_rg, se_re (sqrt of the
    delta-method variances, NaN where negative): unit diagonals (se 0), NaN for a pair that is not in `fit`."""
    out = {k: np.full((T, T), np.nan) for k in ("rg", "re", "se_rg", "se_re")}
    for k in ("rg", "re"):
        np.fill_diagonal(out[k], 1.0)
        np.fill_diagonal(out["se_" + k], 0.0)
    i, j, b = fit["i"], fit["j"], fit[block]
    with np.errstate(invalid="ignore"):
        for k in ("rg", "re"):
            out[k][i, j] = out[k][j, i] = b[k]
            out["se_" + k][i, j] = out["se_" + k][j, i] = np.sqrt(b["var_" + k])
    return out


# ----------------------------------------------------------------------------- B4
ScoreHitsDev = collections.namedtuple("ScoreHitsDev", "snp pheno stats")  # device tensors: int64 (m,), int64 (m,), float64 (m, 3)
ScoreBestDev = collections.namedtuple("ScoreBestDev", "stats snp")       # device tensors: float64 (T, 3), int64 (T,)


def reduce_score_best(blocks, T):
    """The best pair per phenotype over several blocks: blocks is a sequence of (offset, (T,) SCORE_BEST_DTYPE array with snp inside
    the block).  The smallest p_score wins, the smaller snp (offset + row) among equal p_score; a NaN p_score or snp -1 never."""
    out = np.zeros(T, dtype=SCORE_BEST_DTYPE)
    for k in ("beta", "se", "p_score"):
        out[k] = np.nan
    out["snp"] = -1
    for s0, b in blocks:
        snp = np.where(b["snp"] >= 0, b["snp"] + s0, -1)
        p, q = b["p_score"], out["p_score"]
        with np.errstate(invalid="ignore"):
            take = (snp >= 0) & ~np.isnan(p) & ((out["snp"] < 0) | (p < q) | ((p == q) & (snp < out["snp"])))
        new = b[take].copy()
        new["snp"] = snp[take]
        out[take] = new
    return out


class LMM:
    """Mirror of class LMM (src/lmm.h:49-125): the fields CopyFromParam fills (src/lmm.cpp:56-90)
    and the Analyze* drivers.  sumStat is a numpy record array with SUMSTAT's fields."""

    def __init__(self, a_mode=1, l_min=1e-5, l_max=1e5, n_region=10, l_mle_null=0.0, logl_mle_H0=0.0):
        self.a_mode = a_mode
        self.l_min, self.l_max, self.n_region = l_min, l_max, n_region
        self.l_mle_null, self.logl_mle_H0 = l_mle_null, logl_mle_H0
        self.ni_test = 0
        self.n_cvt = 0
        self.time_UtX = 0.0
        self.time_opt = 0.0
        self.sumStat = np.zeros(0, dtype=SUMSTAT_DTYPE)
        self._active = False

    # -- state handling ---------------------------------------------------------------
    def _cfg(self, n, c, plink):
        cfg = L.LmmCfg()
        cfg.a_mode = self.a_mode
        cfg.n, cfg.n_cvt = n, c
        cfg.l_min, cfg.l_max, cfg.n_region = self.l_min, self.l_max, self.n_region
        cfg.l_mle_null, cfg.logl_mle_H0 = self.l_mle_null, self.logl_mle_H0
        cfg.plink_nan_rule = 1 if plink else 0
        return cfg

    def _setup(self, where, U, eval_, UtW, UtY, plink, host, dev):
        """(U, eval, UtW, UtY) to the library: torch device tensors are borrowed in place -- dev(cfg, U, eval, UtW, UtY, stream) --,
        numpy arrays go as contiguous float64 copies -- host(cfg, U, eval, UtW, UtY)."""
        n = U.shape[0]
        if _is_torch(U):
            c = UtW.shape[1] if UtW.dim() == 2 else 1
            self._keep = (U, eval_, UtW, UtY.contiguous())  # borrowed by the library until finish()
            rc = dev(C.byref(self._cfg(n, c, plink)), *[C.c_void_p(t.data_ptr()) for t in self._keep], _stream())
        else:
            UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
            c = UtW.shape[1]
            # converted copies stay bound to a name until the call returns (_ptr keeps only the address)
            arrs = (_np64(np.ascontiguousarray(U), "U"), np.ascontiguousarray(eval_, dtype=np.float64), UtW,
                    np.ascontiguousarray(UtY, dtype=np.float64))
            rc = host(C.byref(self._cfg(n, c, plink)), *[_ptr(a) for a in arrs])
        L.check(rc, where)
        self.ni_test, self.n_cvt = n, c
        self._active = True

    def setup(self, U, eval_, UtW, Uty, plink=False):
        self._setup("LMM.setup", U, eval_, UtW, Uty, plink, L.lib().gemma_hip_lmm_setup, L.lib().gemma_hip_lmm_setup_d)

    def setup_kept(self, UtW, Uty, plink=False):
        """lmm_setup on the kept (U, eval) of EigenDecomp_kept_K (host UtW n x c, Uty n)."""
        n = len(Uty)
        UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
        Uty_c = np.ascontiguousarray(Uty, dtype=np.float64)
        cfg = self._cfg(n, UtW.shape[1], plink)
        L.check(L.lib().gemma_hip_lmm_setup_kept(C.byref(cfg), _ptr(UtW), _ptr(Uty_c)), "LMM.setup_kept")
        self.ni_test, self.n_cvt = n, UtW.shape[1]
        self._active = True

    def set_indicator(self, indicator_idv):
        ind = np.ascontiguousarray(indicator_idv, dtype=np.int32)
        L.check(L.lib().gemma_hip_lmm_set_indicator(_ptr(ind), ind.size), "LMM.set_indicator")

    def batch(self, geno, geno_kind, out=None, l=None, ld=None):
        """One block of SNPs -> SUMSTAT records (numpy in/out, or torch device tensors in/out)."""
        l, ld = _block_dims(geno, geno_kind, l, ld)
        if _is_torch(geno):
            import torch
            if out is None:
                out = torch.empty((l, 8), dtype=torch.float64, device=geno.device)
            rc = L.lib().gemma_hip_lmm_batch_d(geno_kind, C.c_void_p(geno.data_ptr()), l, ld,
                                               C.c_void_p(out.data_ptr()), _stream())
            L.check(rc, "LMM.batch")
            return out
        if out is None:
            out = np.zeros(l, dtype=SUMSTAT_DTYPE)
        L.check(L.lib().gemma_hip_lmm_batch(geno_kind, _ptr(geno), l, ld, _ptr(out)), "LMM.batch")
        return out

    def batch_pipe(self, geno, geno_kind, out):
        """LMM.batch with two blocks in flight (gemma_hip_lmm_batch_pipe_d; torch device tensors): the product of this block beside
        the combine and per-SNP stage of the previous one, on a CU partition.  `out` holds this block's records only after
        pipe_flush() (or any other batch call)."""
        l = geno.shape[0]
        rc = L.lib().gemma_hip_lmm_batch_pipe_d(geno_kind, C.c_void_p(geno.data_ptr()), l, _tld(geno),
                                                C.c_void_p(out.data_ptr()), _stream())
        L.check(rc, "LMM.batch_pipe")
        return out

    def pipe_flush(self):
        L.check(L.lib().gemma_hip_lmm_pipe_flush(_stream()), "LMM.pipe_flush")

    def assoc(self, UtX, out=None):
        """Per-SNP stage only, on a device-resident SNP-major UtX (torch)."""
        import torch
        l = UtX.shape[0]
        if out is None:
            out = torch.empty((l, 8), dtype=torch.float64, device=UtX.device)
        L.check(L.lib().gemma_hip_lmm_assoc_d(C.c_void_p(UtX.data_ptr()), l, _tld(UtX),
                                              C.c_void_p(out.data_ptr()), _stream()), "LMM.assoc")
        return out

    def dbg_utx(self, geno, geno_kind, path):
        """The U^T x stage alone (after setup): (l x n) array, row s = (U^T x_s)^T.  path 0: fp64 MFMA GEMM,
        path 1: exact int8-digit product where the input allows it (PLINK 2-bit, fp64 hard calls, fixed-point dosages);
        last_utx_path() says what ran."""
        geno = np.ascontiguousarray(geno)
        l, ld = geno.shape[0], geno.shape[1]
        if geno_kind == L.GENO_F64_IDV_MAJOR:
            l = geno.shape[1]
        out = np.empty((l, self.ni_test), dtype=np.float64)
        L.check(L.lib().gemma_hip_dbg_utx(geno_kind, _ptr(geno), l, ld, path, _ptr(out)), "LMM.dbg_utx")
        return out

    def finish(self):
        a, b = C.c_double(), C.c_double()
        L.check(L.lib().gemma_hip_lmm_finish(C.byref(a), C.byref(b)), "LMM.finish")
        self.time_UtX, self.time_opt = a.value, b.value
        self._active = False
        self._keep = None

    # -- drivers ----------------------------------------------------------------------
    def Analyze(self, U, eval_, UtW, Uty, geno, geno_kind=L.GENO_F64_SNP_MAJOR, plink=False,
                indicator_idv=None, batch=LMM_BATCH_SIZE):
        """LMM::Analyze (src/lmm.cpp:1474-1658): stream SNP-major `geno` in blocks of LMM_BATCH_SIZE;
        results are appended in SNP order to self.sumStat."""
        outs = _scan(lambda: self.setup(U, eval_, UtW, Uty, plink=plink), self.set_indicator, self.finish, indicator_idv, geno, batch,
                     lambda s0, blk: self.batch(blk, geno_kind))
        self.sumStat = np.concatenate(outs) if outs else np.zeros(0, dtype=SUMSTAT_DTYPE)
        return self.sumStat

    # -- T phenotypes over one U^T x (gemma_hip_lmm_multi_*) ----------------------------
    def setup_multi(self, U, eval_, UtW, UtY, l_mle_null=None, logl_mle_H0=None, plink=False):
        """lmm_setup for the T columns of UtY (n x T) at once: same individuals, kinship and covariates.  l_mle_null /
        logl_mle_H0: T values each (a_mode 2, 3, 4, 9); self.l_mle_null / self.logl_mle_H0 are not read."""
        T = UtY.shape[1]
        nul = None if l_mle_null is None else np.ascontiguousarray(l_mle_null, dtype=np.float64)
        lgl = None if logl_mle_H0 is None else np.ascontiguousarray(logl_mle_H0, dtype=np.float64)
        for v in (nul, lgl):
            if v is not None and v.size != T:
                raise ValueError("LMM.setup_multi: %d null values for %d phenotypes" % (v.size, T))
        pn = _ptr(nul) if nul is not None else None
        pl = _ptr(lgl) if lgl is not None else None
        self._setup("LMM.setup_multi", U, eval_, UtW, UtY, plink,
                    lambda cfg, *arrs: L.lib().gemma_hip_lmm_multi_setup(cfg, T, pn, pl, *arrs),
                    lambda cfg, *arrs: L.lib().gemma_hip_lmm_multi_setup_d(cfg, T, pn, pl, *arrs))
        self.n_ph = T

    def batch_multi(self, geno, geno_kind, out=None, l=None, ld=None):
        """One block of SNPs -> (T, l) SUMSTAT records (numpy), or a (T, l, 8) device tensor (torch): U^T x once, the per-SNP
        stage per phenotype."""
        T = self.n_ph
        l, ld = _block_dims(geno, geno_kind, l, ld)
        if _is_torch(geno):
            import torch
            if out is None:
                out = torch.empty((T, l, 8), dtype=torch.float64, device=geno.device)
            rc = L.lib().gemma_hip_lmm_multi_batch_d(geno_kind, C.c_void_p(geno.data_ptr()), l, ld,
                                                     C.c_void_p(out.data_ptr()), _stream())
            L.check(rc, "LMM.batch_multi")
            return out
        if out is None:
            out = np.zeros((T, l), dtype=SUMSTAT_DTYPE)
        L.check(L.lib().gemma_hip_lmm_multi_batch(geno_kind, _ptr(geno), l, ld, _ptr(out)), "LMM.batch_multi")
        return out

    def AnalyzeMulti(self, U, eval_, UtW, UtY, geno, geno_kind=L.GENO_F64_SNP_MAJOR, plink=False, indicator_idv=None,
                     l_mle_null=None, logl_mle_H0=None, batch=LMM_BATCH_SIZE):
        """LMM::Analyze for every column of UtY (n x T) over ONE pass of the genotypes: returns (and keeps in self.sumStat) a (T, p)
        record array, row t what Analyze gives for UtY[:, t].  Nulls that are not given are fitted in one call (CalcLambdaNullPanel)."""
        UtY = np.ascontiguousarray(UtY, dtype=np.float64).reshape(len(eval_), -1)
        T = UtY.shape[1]
        if l_mle_null is None or logl_mle_H0 is None:
            fits = CalcLambdaNullPanel(eval_, UtW, UtY, self.l_min, self.l_max, self.n_region)
            if l_mle_null is None:
                l_mle_null = fits["l_mle_null"].copy()
            if logl_mle_H0 is None:
                logl_mle_H0 = fits["logl_mle_H0"].copy()
        outs = _scan(lambda: self.setup_multi(U, eval_, UtW, UtY, l_mle_null, logl_mle_H0, plink=plink), self.set_indicator, self.finish,
                     indicator_idv, geno, batch, lambda s0, blk: self.batch_multi(blk, geno_kind))
        self.sumStat = np.concatenate(outs, axis=1) if outs else np.zeros((T, 0), dtype=SUMSTAT_DTYPE)
        return self.sumStat

    # -- score panel: -lmm 3 of T phenotypes from one product per block (gemma_hip_lmm_score_panel_*) --
    def setup_score_panel(self, U, eval_, UtW, UtY, l_mle_null):
        """Score-panel setup for the T columns of UtY (n x T): a_mode must be 3; l_mle_null holds the T null lambdas.  numpy
        arrays are uploaded, torch device tensors are used in place (U, eval: borrowed until finish())."""
        T = UtY.shape[1]
        nul = np.ascontiguousarray(l_mle_null, dtype=np.float64).ravel()
        if nul.size != T:
            raise ValueError("LMM.setup_score_panel: %d null values for %d phenotypes" % (nul.size, T))
        self._setup("LMM.setup_score_panel", U, eval_, UtW, UtY, False,
                    lambda cfg, *arrs: L.lib().gemma_hip_lmm_score_panel_setup(cfg, T, _ptr(nul), *arrs),
                    lambda cfg, *arrs: L.lib().gemma_hip_lmm_score_panel_setup_d(cfg, T, _ptr(nul), *arrs))
        self.n_ph = T

    def batch_score_panel(self, geno, geno_kind, out=None, l=None, ld=None):
        """One block of SNPs -> (T, l) SCORE_DTYPE records (numpy), or a (T, l, 3) device tensor (torch)."""
        T = self.n_ph
        l, ld = _block_dims(geno, geno_kind, l, ld)
        if _is_torch(geno):
            import torch
            if out is None:
                out = torch.empty((T, l, 3), dtype=torch.float64, device=geno.device)
            rc = L.lib().gemma_hip_lmm_score_panel_batch_d(geno_kind, C.c_void_p(geno.data_ptr()), l, ld,
                                                           C.c_void_p(out.data_ptr()), _stream())
            L.check(rc, "LMM.batch_score_panel")
            return out
        if out is None:
            out = np.zeros((T, l), dtype=SCORE_DTYPE)
        L.check(L.lib().gemma_hip_lmm_score_panel_batch(geno_kind, _ptr(geno), l, ld, _ptr(out)), "LMM.batch_score_panel")
        return out

    def assoc_score_panel(self, UtX, out=None):
        """The product alone, on a device-resident SNP-major UtX (torch) -> (T, l, 3) device tensor."""
        import torch
        l = UtX.shape[0]
        if out is None:
            out = torch.empty((self.n_ph, l, 3), dtype=torch.float64, device=UtX.device)
        L.check(L.lib().gemma_hip_lmm_score_panel_assoc_d(C.c_void_p(UtX.data_ptr()), l, _tld(UtX),
                                                          C.c_void_p(out.data_ptr()), _stream()), "LMM.assoc_score_panel")
        return out

    def AnalyzeScorePanel(self, U, eval_, UtW, UtY, geno, geno_kind=L.GENO_F64_SNP_MAJOR, indicator_idv=None, l_mle_null=None,
                          batch=LMM_BATCH_SIZE):
        """`-lmm 3` for every column of UtY (n x T) over ONE pass of the genotypes and one product per block: a (T, p) array of
        (beta, se, p_score) records (numpy in), or a (T, p, 3) device tensor (torch in; l_mle_null is then required).  Nulls that
        are not given are fitted in one call (CalcLambdaNullPanel)."""
        if self.a_mode != 3:
            raise ValueError("LMM.AnalyzeScorePanel: a_mode %d (the score panel is a_mode 3)" % self.a_mode)
        tor = _is_torch(U)
        if not tor:
            UtY = np.ascontiguousarray(UtY, dtype=np.float64).reshape(len(eval_), -1)
        T = UtY.shape[1]
        if l_mle_null is None:
            if tor:
                raise ValueError("LMM.AnalyzeScorePanel: device inputs need l_mle_null")
            l_mle_null = CalcLambdaNullPanel(eval_, UtW, UtY, self.l_min, self.l_max, self.n_region)["l_mle_null"].copy()
        outs = _scan(lambda: self.setup_score_panel(U, eval_, UtW, UtY, l_mle_null), self.set_indicator, self.finish, indicator_idv, geno,
                     batch, lambda s0, blk: self.batch_score_panel(blk, geno_kind))
        if tor:
            import torch
            self.scorePanel = torch.cat(outs, dim=1) if outs else torch.empty((T, 0, 3), dtype=torch.float64, device=U.device)
        else:
            self.scorePanel = np.concatenate(outs, axis=1) if outs else np.zeros((T, 0), dtype=SCORE_DTYPE)
        return self.scorePanel

    # -- the hits form of the score panel: pairs with p_score <= p_max and the best pair per phenotype --
    def _hits_cap(self, l, p_max, cap):
        if cap is not None:
            return int(cap)
        pairs = self.n_ph * l
        return int(min(pairs, max(4096, 2 * p_max * pairs + 1024)))

    def _hits_dev(self, call, l, p_max, cap, device):
        """the torch side of a hits call: call(raw, cap, cnt, best) -> rc; repeats once with a sufficient list"""
        import torch
        T = self.n_ph
        cap = self._hits_cap(l, p_max, cap)
        cnt = torch.zeros(1, dtype=torch.int64, device=device)
        best = torch.empty((T, 4), dtype=torch.int64, device=device)
        while True:
            raw = torch.empty((max(cap, 1), 4), dtype=torch.int64, device=device)
            L.check(call(C.c_void_p(raw.data_ptr()) if cap else None, cap, C.c_void_p(cnt.data_ptr()), C.c_void_p(best.data_ptr())),
                    "LMM.score_panel_hits")
            n = int(cnt.item())
            if n <= cap:
                break
            cap = n
        raw = raw[:n]
        key = raw[:, 0]  # snp in the low, pheno in the high 32 bits
        snp, pheno = key & 0xffffffff, (key >> 32) & 0xffffffff
        order = torch.argsort((pheno << 32) | snp)
        hits = ScoreHitsDev(snp[order], pheno[order], raw[:, 1:].contiguous().view(torch.float64)[order])
        return hits, ScoreBestDev(best[:, :3].contiguous().view(torch.float64), best[:, 3].clone())

    # -- the refinement of the hits: each pair's own lambda-hats, Wald and LRT (gemma_hip_lmm_score_panel_refine_*) --
    def setup_score_refine(self, UtY, logl_mle_H0):
        """After setup_score_panel: keeps what the refinement of hit pairs needs, a transposed copy of UtY (n x T) and the T
        logl_mle_H0 of the null fits (CalcLambdaNullPanel).  numpy arrays are uploaded, a torch device UtY is read in place."""
        T = self.n_ph
        logl = np.ascontiguousarray(logl_mle_H0, dtype=np.float64).ravel()
        if logl.size != T or UtY.shape[1] != T:
            raise ValueError("LMM.setup_score_refine: %d null values and %d columns for %d phenotypes" % (logl.size, UtY.shape[1], T))
        if _is_torch(UtY):
            UtY = UtY.contiguous()
            rc = L.lib().gemma_hip_lmm_score_panel_refine_setup_d(C.c_void_p(UtY.data_ptr()), _ptr(logl), _stream())
        else:
            UtY = np.ascontiguousarray(UtY, dtype=np.float64)
            rc = L.lib().gemma_hip_lmm_score_panel_refine_setup(_ptr(UtY), _ptr(logl))
        L.check(rc, "LMM.setup_score_refine")

    @staticmethod
    def _pairs_dev(hits, device):
        """ScoreHitsDev or an (m, 2) integer tensor of (snp, pheno) -> (m, 4) int64: gemma_score_hit entries with the key filled in"""
        import torch
        if isinstance(hits, ScoreHitsDev):
            snp, pheno = hits.snp, hits.pheno
        else:
            hits = torch.as_tensor(hits, device=device)
            if hits.dim() != 2 or hits.shape[1] != 2 or hits.dtype.is_floating_point:
                raise ValueError("LMM refinement: pairs are a ScoreHitsDev or an (m, 2) integer tensor of (snp, pheno)")
            snp, pheno = hits[:, 0], hits[:, 1]
        snp, pheno = snp.to(device=device, dtype=torch.int64), pheno.to(device=device, dtype=torch.int64)
        if len(snp) and (int(snp.min()) < 0 or int(pheno.min()) < 0 or int(snp.max()) > 0xffffffff or int(pheno.max()) > 0xffffffff):
            raise ValueError("LMM refinement: snp and pheno are unsigned 32-bit indices")
        raw = torch.zeros((len(snp), 4), dtype=torch.int64, device=device)
        raw[:, 0] = snp | (pheno << 32)  # snp in the low, pheno in the high 32 bits
        return raw

    def assoc_score_refine(self, UtX, hits):
        """The `-lmm 4` records of the pairs in `hits` (ScoreHitsDev, or an (m, 2) integer tensor of (snp, pheno)) on a
        device-resident SNP-major UtX (torch) -> (m, 8) device tensor in SUMSTAT order, row i for pair i.  A pair outside the block
        or the panel gets NaN."""
        import torch
        raw = self._pairs_dev(hits, UtX.device)
        out = torch.empty((raw.shape[0], 8), dtype=torch.float64, device=UtX.device)
        L.check(L.lib().gemma_hip_lmm_score_panel_refine_assoc_d(C.c_void_p(UtX.data_ptr()), UtX.shape[0], _tld(UtX),
                                                                 C.c_void_p(raw.data_ptr()), raw.shape[0], C.c_void_p(out.data_ptr()),
                                                                 _stream()), "LMM.assoc_score_refine")
        return out

    def refine_last(self, hits, device="cuda"):
        """assoc_score_refine on the U^T x of the most recent batch_score_panel / batch_score_panel_hits of this setup."""
        import torch
        if isinstance(hits, ScoreHitsDev):
            device = hits.snp.device
        elif _is_torch(hits):
            device = hits.device if hits.is_cuda else device
        raw = self._pairs_dev(hits, device)
        out = torch.empty((raw.shape[0], 8), dtype=torch.float64, device=raw.device)
        L.check(L.lib().gemma_hip_lmm_score_panel_refine_last_d(C.c_void_p(raw.data_ptr()), raw.shape[0], C.c_void_p(out.data_ptr()),
                                                                _stream()), "LMM.refine_last")
        return out

    def batch_score_panel_hits(self, geno, geno_kind, p_max, cap=None, refine=False):
        """One block of SNPs -> (hits, best).  numpy in: hits is a SCORE_HIT_DTYPE array of every pair with p_score <= p_max, sorted
        by (pheno, snp), snp the row inside the block; best a (T,) SCORE_BEST_DTYPE array (snp -1, NaN: no pair).  torch in:
        ScoreHitsDev(snp, pheno, stats (m, 3)) and ScoreBestDev(stats (T, 3), snp) of device tensors, sorted the same way.  cap: the
        size of the first list; a block with more hits is run again with a list that holds them.
        refine=True (after setup_score_refine) -> (hits, best, refined): the `-lmm 4` record of every hit, aligned with hits -- a
        SUMSTAT_DTYPE array (numpy in) or an (m, 8) device tensor (torch in)."""
        T = self.n_ph
        p_max = float(p_max)
        l, ld = _block_dims(geno, geno_kind)
        if _is_torch(geno):
            gp, st = C.c_void_p(geno.data_ptr()), _stream()
            hits, best = self._hits_dev(lambda raw, cap_, cnt, best: L.lib().gemma_hip_lmm_score_panel_hits_batch_d(
                geno_kind, gp, l, ld, p_max, raw, cap_, cnt, best, st), l, p_max, cap, geno.device)
            return (hits, best, self.refine_last(hits)) if refine else (hits, best)
        cap = self._hits_cap(l, p_max, cap)
        best = np.zeros(T, dtype=SCORE_BEST_DTYPE)
        cnt = C.c_ulonglong(0)
        while refine:
            hits, refined = np.zeros(cap, dtype=SCORE_HIT_DTYPE), np.zeros(cap, dtype=SUMSTAT_DTYPE)
            L.check(L.lib().gemma_hip_lmm_score_panel_hits_refine_batch(
                geno_kind, _ptr(geno), l, ld, p_max, _ptr(hits) if cap else None, cap, C.cast(C.byref(cnt), C.c_void_p), _ptr(best),
                _ptr(refined) if cap else None), "LMM.batch_score_panel_hits")
            if cnt.value <= cap:
                return hits[:cnt.value], best, refined[:cnt.value]
            cap = int(cnt.value)
        while True:
            hits = np.zeros(cap, dtype=SCORE_HIT_DTYPE)
            L.check(L.lib().gemma_hip_lmm_score_panel_hits_batch(geno_kind, _ptr(geno), l, ld, p_max, _ptr(hits) if cap else None, cap,
                                                                 C.cast(C.byref(cnt), C.c_void_p), _ptr(best)), "LMM.batch_score_panel_hits")
            if cnt.value <= cap:
                return hits[:cnt.value], best
            cap = int(cnt.value)

    def assoc_score_panel_hits(self, UtX, p_max, cap=None):
        """The hits form of the product alone, on a device-resident SNP-major UtX (torch): as batch_score_panel_hits for torch."""
        l, ld, p_max = UtX.shape[0], _tld(UtX), float(p_max)
        xp, st = C.c_void_p(UtX.data_ptr()), _stream()
        return self._hits_dev(lambda raw, cap_, cnt, best: L.lib().gemma_hip_lmm_score_panel_hits_assoc_d(
            xp, l, ld, p_max, raw, cap_, cnt, best, st), l, p_max, cap, UtX.device)

    def AnalyzeScorePanelHits(self, U, eval_, UtW, UtY, geno, geno_kind=L.GENO_F64_SNP_MAJOR, p_max=1e-5, indicator_idv=None,
                              l_mle_null=None, batch=LMM_BATCH_SIZE, refine=False, logl_mle_H0=None):
        """AnalyzeScorePanel without the (T, p) records: one pass over the genotypes -> (hits, best) as batch_score_panel_hits gives
        them, with snp the index over the whole scan (block offset + row); best is reduced over the blocks (the smallest p_score,
        the smaller snp among equals, NaN never).  Nulls are fitted as AnalyzeScorePanel fits them.
        refine=True -> (hits, best, refined): the `-lmm 4` record of every hit (its own lambda-hats, Wald, LRT), aligned with hits;
        logl_mle_H0 are the T null log-likelihoods, fitted with the lambdas where either is missing."""
        if self.a_mode != 3:
            raise ValueError("LMM.AnalyzeScorePanelHits: a_mode %d (the score panel is a_mode 3)" % self.a_mode)
        tor = _is_torch(U)
        if not tor:
            UtY = np.ascontiguousarray(UtY, dtype=np.float64).reshape(len(eval_), -1)
        T = UtY.shape[1]
        if l_mle_null is None:
            if tor:
                raise ValueError("LMM.AnalyzeScorePanelHits: device inputs need l_mle_null")
            l_mle_null = CalcLambdaNullPanel(eval_, UtW, UtY, self.l_min, self.l_max, self.n_region)["l_mle_null"].copy()
        if refine and logl_mle_H0 is None:
            if tor:
                raise ValueError("LMM.AnalyzeScorePanelHits: device inputs need logl_mle_H0")
            logl_mle_H0 = CalcLambdaNullPanel(eval_, UtW, UtY, self.l_min, self.l_max, self.n_region)["logl_mle_H0"].copy()
        outs = _scan(lambda: self.setup_score_panel(U, eval_, UtW, UtY, l_mle_null), self.set_indicator, self.finish, indicator_idv, geno,
                     batch, lambda s0, blk: (s0,) + self.batch_score_panel_hits(blk, geno_kind, p_max, refine=refine),
                     prepare=(lambda: self.setup_score_refine(UtY, logl_mle_H0)) if refine else None)
        parts, bests = [(s0, o[0]) for s0, *o in outs], [(s0, o[1]) for s0, *o in outs]
        refs = [o[2] for _, *o in outs] if refine else None
        if tor:
            import torch
            dev = U.device
            if parts:
                hits = ScoreHitsDev(torch.cat([h.snp + s0 for s0, h in parts]), torch.cat([h.pheno for _, h in parts]),
                                    torch.cat([h.stats for _, h in parts]))
                order = torch.argsort((hits.pheno << 32) | hits.snp)
                hits = ScoreHitsDev(hits.snp[order], hits.pheno[order], hits.stats[order])
                refined = torch.cat(refs)[order] if refine else None
            else:
                hits = ScoreHitsDev(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                                    torch.empty((0, 3), dtype=torch.float64, device=dev))
                refined = torch.empty((0, 8), dtype=torch.float64, device=dev)
            stats = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)
            snp = torch.full((T,), -1, dtype=torch.int64, device=dev)
            for s0, b in bests:
                bs = torch.where(b.snp >= 0, b.snp + s0, b.snp)
                p, q = b.stats[:, 2], stats[:, 2]
                take = (bs >= 0) & ~torch.isnan(p) & ((snp < 0) | (p < q) | ((p == q) & (bs < snp)))
                stats = torch.where(take[:, None], b.stats, stats)
                snp = torch.where(take, bs, snp)
            best = ScoreBestDev(stats, snp)
        else:
            hits = np.concatenate([h for _, h in parts]) if parts else np.zeros(0, dtype=SCORE_HIT_DTYPE)
            off = np.concatenate([np.full(len(h), s0, dtype=np.uint32) for s0, h in parts]) if parts else np.zeros(0, dtype=np.uint32)
            hits["snp"] += off
            order = np.lexsort((hits["snp"], hits["pheno"]))
            hits = hits[order]
            refined = (np.concatenate(refs) if refs else np.zeros(0, dtype=SUMSTAT_DTYPE))[order] if refine else None
            best = reduce_score_best(bests, T)
        self.scoreHits, self.scoreBest = hits, best
        if refine:
            self.scoreRefined = refined
            return hits, best, refined
        return hits, best

    def AnalyzeBimbam(self, U, eval_, UtW, Uty, X_snpmajor_nan):
        """src/lmm.cpp:1660-1706 with the file reader factored out: X is SNP-major over the analysed
        individuals, NaN = "NA"."""
        return self.Analyze(U, eval_, UtW, Uty, np.ascontiguousarray(X_snpmajor_nan, dtype=np.float64),
                            L.GENO_F64_SNP_MAJOR, plink=False)

    def AnalyzeGene(self, U, eval_, UtW, Utx, Y, batch=LMM_BATCH_SIZE):
        """LMM::AnalyzeGene (src/lmm.cpp:1365-1471): Y (genes x n) holds one phenotype per row, Utx = U^T x is the
        fixed tested variable; every row gets its own null fit (l_H0, logl_H0)."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        self.setup(U, eval_, UtW, Utx)
        try:
            outs = []
            for s0 in range(0, Y.shape[0], batch):
                blk = Y[s0:s0 + batch]
                out = np.zeros(blk.shape[0], dtype=SUMSTAT_DTYPE)
                L.check(L.lib().gemma_hip_lmm_gene_batch(_ptr(blk), blk.shape[0], blk.shape[1], _ptr(out)),
                        "LMM.AnalyzeGene")
                outs.append(out)
        finally:
            self.finish()
        self.sumStat = np.concatenate(outs) if outs else np.zeros(0, dtype=SUMSTAT_DTYPE)
        return self.sumStat

    def AnalyzeGXE(self, U, eval_, UtW, Uty, env, geno, geno_kind=L.GENO_F64_SNP_MAJOR, indicator_idv=None,
                   batch=LMM_BATCH_SIZE):
        """LMM::AnalyzeBimbamGXE / AnalyzePlinkGXE (src/lmm.cpp:2283-2608): covariates [W, env, x_s], tested variable
        x_s . env; env is over the analysed individuals."""
        plink = geno_kind == L.GENO_PLINK_2BIT
        env = np.ascontiguousarray(env, dtype=np.float64)

        def block(s0, blk):
            l, ld = _block_dims(blk, geno_kind)
            out = np.zeros(l, dtype=SUMSTAT_DTYPE)
            L.check(L.lib().gemma_hip_lmm_gxe_batch(geno_kind, _ptr(blk), l, ld, _ptr(out)), "LMM.AnalyzeGXE")
            return out
        outs = _scan(lambda: self.setup(U, eval_, UtW, Uty, plink=plink), self.set_indicator, self.finish, indicator_idv,
                     np.ascontiguousarray(geno), batch, block,
                     prepare=lambda: L.check(L.lib().gemma_hip_lmm_set_env(_ptr(env)), "LMM.set_env"))
        self.sumStat = np.concatenate(outs) if outs else np.zeros(0, dtype=SUMSTAT_DTYPE)
        return self.sumStat

    def AnalyzePlink(self, U, eval_, UtW, Uty, bed_rows, indicator_idv):
        """src/lmm.cpp:1710-1903: bed_rows = the .bed payload of the analysed SNPs (uint8, one row of
        ceil(ni_total/4) bytes per SNP); non-analysed individuals are dropped on device."""
        return self.Analyze(U, eval_, UtW, Uty, np.ascontiguousarray(bed_rows, dtype=np.uint8),
                            L.GENO_PLINK_2BIT, plink=True, indicator_idv=indicator_idv)

    def WriteFiles(self, path, snp_info):
        """LMM::WriteFiles (src/lmm.cpp:101-225): `.assoc.txt`.  snp_info: iterable of dicts with
        chr, rs, ps, n_miss, allele1, allele0, af for every analysed SNP, in order."""
        m = self.a_mode
        head = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\t"
        cols = {1: ["beta", "se", "logl_H1", "l_remle", "p_wald"],
                2: ["logl_H1", "l_mle", "p_lrt"],
                3: ["beta", "se", "p_score"],
                4: ["beta", "se", "logl_H1", "l_remle", "l_mle", "p_wald", "p_lrt", "p_score"],
                9: ["beta", "se", "l_mle", "p_lrt"]}[m]
        field = {"l_remle": "lambda_remle", "l_mle": "lambda_mle"}
        with open(path, "w") as f:
            f.write(head + "\t".join(cols) + "\n")
            for info, st in zip(snp_info, self.sumStat):
                f.write("%s\t%s\t%s\t%d\t%s\t%s\t%.3f" % (info["chr"], info["rs"], info["ps"], info["n_miss"],
                                                          info["allele1"], info["allele0"], info["af"]))
                for cname in cols:
                    f.write("\t%.6e" % st[field.get(cname, cname)])
                f.write("\n")


class LM:
    """Mirror of class LM (src/lm.h) for `-lm 1..4` (a_mode 51..54): ordinary per-SNP regression, no kinship."""

    def __init__(self, a_mode=51):
        self.a_mode = a_mode
        self.sumStat = np.zeros(0, dtype=SUMSTAT_DTYPE)

    def Analyze(self, W, y, geno, geno_kind=L.GENO_F64_SNP_MAJOR, indicator_idv=None, batch=LMM_BATCH_SIZE):
        """LM::AnalyzeBimbam / AnalyzePlink (src/lm.cpp:382-640) over SNP-major `geno`."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64).reshape(len(y), -1)
        geno = np.ascontiguousarray(geno)  # SNP-major rows (a Fortran-ordered array would hand over a stride of 1)

        def set_indicator(indicator_idv):
            ind = np.ascontiguousarray(indicator_idv, dtype=np.int32)
            L.check(L.lib().gemma_hip_lmm_set_indicator(_ptr(ind), ind.size), "LM.set_indicator")

        def block(s0, blk):
            l, ld = _block_dims(blk, geno_kind)
            out = np.zeros(l, dtype=SUMSTAT_DTYPE)
            L.check(L.lib().gemma_hip_lm_batch(geno_kind, _ptr(blk), l, ld, _ptr(out)), "LM.batch")
            return out
        outs = _scan(lambda: L.check(L.lib().gemma_hip_lm_setup(self.a_mode, W.shape[0], W.shape[1], _ptr(W), _ptr(y)), "LM.setup"),
                     set_indicator, lambda: L.check(L.lib().gemma_hip_lm_finish(), "LM.finish"), indicator_idv, geno, batch, block)
        self.sumStat = np.concatenate(outs) if outs else np.zeros(0, dtype=SUMSTAT_DTYPE)
        return self.sumStat


class MVLMM:
    """Mirror of class MVLMM (src/mvlmm.h:32-104): the fields CopyFromParam fills (src/mvlmm.cpp:51-90) and
    AnalyzeBimbam / AnalyzePlink (:2972-3899); crt = 1 is the reference's -crt (CalcCRT / PCRT).  sumStat is a dict of arrays with MPHSUMSTAT's fields
    (src/param.h:68-77): beta (l x d), Vbeta / Vg / Ve (l x d(d+1)/2, upper triangles row by row), p_wald, p_lrt, p_score."""

    def __init__(self, a_mode=1, l_min=1e-5, l_max=1e5, n_region=10, em_iter=10000, nr_iter=100, em_prec=1e-4,
                 nr_prec=1e-4, p_nr=1e-3, crt=0):
        self.a_mode = a_mode
        self.crt = crt
        self.l_min, self.l_max, self.n_region = l_min, l_max, n_region
        self.em_iter, self.nr_iter, self.em_prec, self.nr_prec, self.p_nr = em_iter, nr_iter, em_prec, nr_prec, p_nr
        self.sumStat = {}
        self.null = None

    def _opt(self, gxe=0):
        return L.MvOpt(self.em_iter, self.nr_iter, self.em_prec, self.nr_prec, self.p_nr, self.crt, gxe)

    def fit_null(self, eval_, UtW, UtY, want_se=False):
        """The null block (src/mvlmm.cpp:3056-3208) -> dict with Vg/Ve/B/logl for 'remle' and 'mle'; also fills the
        members WriteFiles' callers read (Vg_remle_null, ..., logl_mle_H0).  want_se: the same fit (the same bits) through
        gemma_hip_mvlmm_null_se, and the dict also holds the VARIANCES VVg_*, VVe_* (v = d (d + 1) / 2, upper triangle row by row)
        and VB_* (d x c) whose safe_sqrt the reference prints as se(Vg), se(Ve) and se(B) (:3106-3128)."""
        UtY = np.ascontiguousarray(UtY, dtype=np.float64)
        n, d = UtY.shape
        UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
        c = UtW.shape[1]
        ev = np.ascontiguousarray(eval_, dtype=np.float64)
        nf, opt = L.MvNull(), self._opt()
        if want_se:
            se = L.MvNullSe()
            L.check(L.lib().gemma_hip_mvlmm_null_se(n, c, d, _ptr(ev), _ptr(UtW), _ptr(UtY), self.l_min, self.l_max,
                                                    self.n_region, C.byref(opt), C.byref(nf), C.byref(se)), "MVLMM.fit_null")
        else:
            L.check(L.lib().gemma_hip_mvlmm_null(n, c, d, _ptr(ev), _ptr(UtW), _ptr(UtY), self.l_min, self.l_max,
                                                 self.n_region, C.byref(opt), C.byref(nf)), "MVLMM.fit_null")
        self._null_struct = nf
        g = lambda a, r, k: np.array(a[:r * k]).reshape(r, k)
        self.null = {"Vg_remle": g(nf.Vg_remle, d, d), "Ve_remle": g(nf.Ve_remle, d, d), "B_remle": g(nf.B_remle, d, c),
                     "logl_remle": nf.logl_remle_H0, "Vg_mle": g(nf.Vg_mle, d, d), "Ve_mle": g(nf.Ve_mle, d, d),
                     "B_mle": g(nf.B_mle, d, c), "logl_mle": nf.logl_mle_H0}
        if want_se:
            v = d * (d + 1) // 2
            for tag in ("remle", "mle"):
                self.null["VVg_" + tag] = np.array(getattr(se, "VVg_" + tag)[:v])
                self.null["VVe_" + tag] = np.array(getattr(se, "VVe_" + tag)[:v])
                self.null["VB_" + tag] = g(getattr(se, "VB_" + tag), d, c)
        self.logl_remle_H0, self.logl_mle_H0 = nf.logl_remle_H0, nf.logl_mle_H0
        return self.null

    def Analyze(self, U, eval_, UtW, UtY, geno, geno_kind, indicator_idv=None, batch=LMM_BATCH_SIZE, env=None):
        """env (over the analysed individuals): the interaction test of AnalyzeBimbamGXE / AnalyzePlinkGXE (src/mvlmm.cpp:3970-4870):
        the null model is fitted on (W, env) (:4046-4070), per SNP x o env is tested with (W, env, x) as covariates."""
        UtY = np.ascontiguousarray(UtY, dtype=np.float64)
        n, d = UtY.shape
        UtW = np.ascontiguousarray(UtW, dtype=np.float64).reshape(n, -1)
        if env is not None:
            env = np.ascontiguousarray(env, dtype=np.float64)
            Ute = CalcUtX(np.ascontiguousarray(U, dtype=np.float64), env)  # gsl_blas_dgemv(CblasTrans, U, env), :4047 -- on the library's GEMM
            self.fit_null(eval_, np.column_stack([UtW, Ute]), UtY)
        else:
            self.fit_null(eval_, UtW, UtY)
        lmm = LMM(a_mode=self.a_mode, l_min=self.l_min, l_max=self.l_max, n_region=self.n_region)
        lmm.setup(U, eval_, UtW, np.ascontiguousarray(UtY[:, 0]), plink=(geno_kind == L.GENO_PLINK_2BIT))
        v = d * (d + 1) // 2
        stride = d + 3 * v + 3
        outs = []
        try:
            if indicator_idv is not None:
                lmm.set_indicator(indicator_idv)
            if env is not None:
                L.check(L.lib().gemma_hip_lmm_set_env(_ptr(env)), "MVLMM.set_env")
            opt = self._opt(gxe=1 if env is not None else 0)
            L.check(L.lib().gemma_hip_mvlmm_set(d, _ptr(UtY), C.byref(self._null_struct), C.byref(opt)), "MVLMM.set")
            geno = np.ascontiguousarray(geno)
            for s0 in range(0, geno.shape[0], batch):
                blk = geno[s0:s0 + batch]
                l, ld = _block_dims(blk, geno_kind)
                out = np.zeros((l, stride))
                L.check(L.lib().gemma_hip_mvlmm_batch(geno_kind, _ptr(blk), l, ld, _ptr(out)), "MVLMM.Analyze")
                outs.append(out)
        finally:
            lmm.finish()
        o = np.concatenate(outs) if outs else np.zeros((0, stride))
        self.sumStat = {"beta": o[:, :d], "Vbeta": o[:, d:d + v], "Vg": o[:, d + v:d + 2 * v],
                        "Ve": o[:, d + 2 * v:d + 3 * v], "p_wald": o[:, d + 3 * v], "p_lrt": o[:, d + 3 * v + 1],
                        "p_score": o[:, d + 3 * v + 2]}
        return self.sumStat

    def AnalyzeBimbam(self, U, eval_, UtW, UtY, X_snpmajor, batch=LMM_BATCH_SIZE):
        """src/mvlmm.cpp:2972-3416: X_snpmajor holds one row per analysed SNP over the analysed individuals, NaN = NA."""
        return self.Analyze(U, eval_, UtW, UtY, np.ascontiguousarray(X_snpmajor, dtype=np.float64), L.GENO_F64_SNP_MAJOR,
                            batch=batch)

    def AnalyzePlink(self, U, eval_, UtW, UtY, bed_rows, indicator_idv, batch=LMM_BATCH_SIZE):
        """src/mvlmm.cpp:3418-3899"""
        return self.Analyze(U, eval_, UtW, UtY, np.ascontiguousarray(bed_rows, dtype=np.uint8), L.GENO_PLINK_2BIT,
                            indicator_idv=indicator_idv, batch=batch)

    def AnalyzeBimbamGXE(self, U, eval_, UtW, UtY, env, X_snpmajor, batch=LMM_BATCH_SIZE):
        """src/mvlmm.cpp:3970-4414"""
        return self.Analyze(U, eval_, UtW, UtY, np.ascontiguousarray(X_snpmajor, dtype=np.float64), L.GENO_F64_SNP_MAJOR,
                            batch=batch, env=env)

    def AnalyzePlinkGXE(self, U, eval_, UtW, UtY, env, bed_rows, indicator_idv, batch=LMM_BATCH_SIZE):
        """src/mvlmm.cpp:4416-4870"""
        return self.Analyze(U, eval_, UtW, UtY, np.ascontiguousarray(bed_rows, dtype=np.uint8), L.GENO_PLINK_2BIT,
                            indicator_idv=indicator_idv, batch=batch, env=env)

    def WriteFiles(self, path, snp_info):
        """MVLMM::WriteFiles (src/mvlmm.cpp:117-210)"""
        d = self.sumStat["beta"].shape[1]
        head = ["chr", "rs", "ps", "n_miss", "allele1", "allele0", "af"] + ["beta_%d" % (i + 1) for i in range(d)]
        head += ["Vbeta_%d_%d" % (i + 1, j + 1) for i in range(d) for j in range(i, d)]
        pcols = {1: ["p_wald"], 2: ["p_lrt"], 3: ["p_score"], 4: ["p_wald", "p_lrt", "p_score"]}[self.a_mode]
        with open(path, "w") as f:
            f.write("\t".join(head + pcols) + "\n")
            for t, si in enumerate(snp_info):
                row = [str(si["chr"]), str(si["rs"]), str(si["ps"]), str(si["n_miss"]), str(si["allele1"]),
                       str(si["allele0"]), "%.3f" % si["af"]]
                row += ["%.6e" % x for x in self.sumStat["beta"][t]] + ["%.6e" % x for x in self.sumStat["Vbeta"][t]]
                row += ["%.6e" % self.sumStat[k][t] for k in pcols]
                f.write("\t".join(row) + "\n")


# ----------------------------------------------------------------------------- variance components (-vc 1 / -vc 2)
def _torch_square_f64(t, name):
    import torch
    if t.dtype != torch.float64 or not t.is_cuda or t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError("%s must be a square float64 CUDA tensor" % name)
    return t


def spd_inverse(A, return_logdet=False):
    """Inverse of a symmetric positive-definite matrix (a new array; torch device tensors in place), and log det A.
    Raises GemmaHipError with code ENOTPD on the first pivot that is not > 0 (the reference's LU would carry on); the
    error's `bad_pivot` holds that pivot's 0-based index."""
    ld, bad = C.c_double(0.0), C.c_long(-1)
    try:
        if _is_torch(A):
            import torch
            _torch_square_f64(A, "A")
            # the library works on the stream it is handed: torch's current one
            L.check(L.lib().gemma_hip_spd_inverse_d(C.c_void_p(A.data_ptr()), A.shape[0], _tld(A), C.byref(ld), C.byref(bad),
                                                    _stream()), "spd_inverse")
            out = A
        else:
            out = np.array(_np64(np.asarray(A), "A"), dtype=np.float64, order="C", copy=True)
            if out.ndim != 2 or out.shape[0] != out.shape[1]:
                raise ValueError("A must be square")
            L.check(L.lib().gemma_hip_spd_inverse(_ptr(out), out.shape[0], out.shape[0], C.byref(ld), C.byref(bad)),
                    "spd_inverse")
    except L.GemmaHipError as e:
        e.bad_pivot = bad.value if e.code == L.ENOTPD else None
        raise
    return (out, ld.value) if return_logdet else out


class VC:
    """Mirror of class VC (src/vc.h): CalcVChe (-vc 1) and CalcVCreml (-vc 2) on one or more kinships.  Ks are the kinships
    as src/gemma.cpp:2328-2369 hands them over (centred by CenterMatrix(G); v_traceG = their mean diagonals), numpy arrays
    (copied to the device) or torch device tensors (used in place).  After a call the fields v_sigma2, v_se_sigma2, v_pve,
    v_se_pve, pve_total, se_pve_total (and for REML iterations, status, evaluations, inverses, iter_sigma2, timing) hold the fit."""

    def _setup(self, Ks, W, y):
        Ks = list(Ks)
        n = Ks[0].shape[0]
        self._W = np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(n, -1))
        self._y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(n))
        self.n_vc = len(Ks)
        arr = (C.c_void_p * self.n_vc)()
        if _is_torch(Ks[0]):
            import torch
            ldk = _tld(Ks[0])
            for i, K in enumerate(Ks):
                _torch_square_f64(K, "kinship %d" % i)
                if K.shape[0] != n or _tld(K) != ldk:
                    raise ValueError("kinships must be n x n and share one leading dimension")
                arr[i] = K.data_ptr()
            fn = L.lib().gemma_hip_vc_setup_d
            self._keep = Ks
            torch.cuda.current_stream().synchronize()  # the fit runs on the null stream: the kinships must be complete
        else:
            self._keep = [np.ascontiguousarray(_np64(np.asarray(K), "K")) for K in Ks]
            ldk = n
            for i, K in enumerate(self._keep):
                if K.shape != (n, n):
                    raise ValueError("kinship %d is not %d x %d" % (i, n, n))
                arr[i] = K.ctypes.data
            fn = L.lib().gemma_hip_vc_setup
        L.check(fn(n, self.n_vc, C.cast(arr, C.POINTER(C.c_void_p)), ldk, _ptr(self._W), self._W.shape[1], _ptr(self._y)),
                "vc_setup")

    def _outs(self):
        m = self.n_vc
        return np.zeros(m + 1), np.zeros(m + 1), np.zeros(m), np.zeros(m), C.c_double(0.0), C.c_double(0.0)

    def _store(self, s2, se2, pve, sepve, pt, sept):
        self.v_sigma2, self.v_se_sigma2, self.v_pve, self.v_se_pve = s2, se2, pve, sepve
        self.pve_total, self.se_pve_total = pt.value, sept.value

    def CalcVChe(self, Ks, W, y):
        """src/vc.cpp:1503-1724"""
        self._setup(Ks, W, y)
        try:
            o = self._outs()
            L.check(L.lib().gemma_hip_vc_he(_ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), C.byref(o[4]), C.byref(o[5])), "vc_he")
            self._store(*o)
        finally:
            L.lib().gemma_hip_vc_release()
        return self

    def CalcVCreml(self, Ks, W, y, noconstrain=False):
        """src/vc.cpp:1726-1931"""
        self._setup(Ks, W, y)
        try:
            o = self._outs()
            it, st, cnt = C.c_int(0), C.c_int(0), (C.c_long * 2)()
            trace = np.zeros((102, self.n_vc + 1))
            L.check(L.lib().gemma_hip_vc_reml(1 if noconstrain else 0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]),
                                              C.byref(o[4]), C.byref(o[5]), C.byref(it), C.byref(st), cnt, _ptr(trace),
                                              trace.shape[0]), "vc_reml")
            self._store(*o)
            self.iterations, self.status = it.value, st.value
            self.evaluations, self.inverses = cnt[0], cnt[1]
            self.iter_sigma2 = trace[:it.value + 1].copy()
            t5 = np.zeros(5)
            L.check(L.lib().gemma_hip_vc_timing(_ptr(t5)), "vc_timing")
            self.timing = dict(zip(("assembly", "spd_inverse", "p_correction", "matvec", "trace"), t5.tolist()))
        finally:
            L.lib().gemma_hip_vc_release()
        return self


# ----------------------------------------------------------------------------- genomic prediction (-bslmm 2, -predict 1 / 2)
def _g6(v):
    """A double as the reference's default stream precision prints it (`outfile << d`: %g with six significant digits)."""
    return "%g" % v


def _blocks(geno, batch):
    geno = np.ascontiguousarray(geno)
    for s0 in range(0, geno.shape[0], batch):
        yield geno[s0:s0 + batch]


def ridge_set_r(r, scale=1.0):
    """gemma_hip_ridge_set_r: the vector of the genotype product as it is (ridge_batch then returns scale * X_c' r)."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    L.check(L.lib().gemma_hip_ridge_set_r(r.size, _ptr(r), scale), "ridge_set_r")


def ridge_set_indicator(indicator_idv):
    ind = np.ascontiguousarray(indicator_idv, dtype=np.int32)
    L.check(L.lib().gemma_hip_ridge_set_indicator(_ptr(ind), ind.size), "ridge_set_indicator")


def ridge_batch(geno, geno_kind, out=None):
    """One block of SNP-major rows -> alpha (numpy in / out, or torch device tensors in / out on torch's current stream)."""
    l = geno.shape[0]
    if _is_torch(geno):
        import torch
        if out is None:
            out = torch.empty(l, dtype=torch.float64, device=geno.device)
        L.check(L.lib().gemma_hip_ridge_batch_d(geno_kind, C.c_void_p(geno.data_ptr()), l, _tld(geno), C.c_void_p(out.data_ptr()),
                                                _stream()), "ridge_batch")
        return out
    geno = np.ascontiguousarray(geno)
    if out is None:
        out = np.zeros(l)
    L.check(L.lib().gemma_hip_ridge_batch(geno_kind, _ptr(geno), l, _row_ld(geno) if l else 0, _ptr(out)),
            "ridge_batch")
    return out


def ridge_finish():
    L.check(L.lib().gemma_hip_ridge_finish(), "ridge_finish")


class BSLMM:
    """Mirror of class BSLMM (src/bslmm.h) for its deterministic mode, `-bslmm 2` (a_mode 12): RidgeR, WriteParam, WriteBV, and the
    fields of the summary the reference logs for the fit (src/gemma.cpp:2938-2946, :2885; PARAM::pheno_mean)."""

    def __init__(self):
        self.a_mode = 12
        self.alpha = np.zeros(0)
        self.bv = np.zeros(0)
        self.pheno_mean = 0.0
        self.l_remle_null = self.pve_null = self.pve_se_null = float("nan")

    def FitNull(self, eval_, UtW, Uty, trace_G, pheno_mean=0.0, l_min=1e-5, l_max=1e5, n_region=10):
        """CalcLambda 'R' + CalcPve of the call site (src/gemma.cpp:2939-2944) on the library's null fit; pheno_mean is what
        CenterVector(y) returned (:2885).  Returns lambda."""
        nf = CalcLambdaNull(eval_, UtW, Uty, l_min, l_max, n_region, trace_G)
        self.l_remle_null, self.pve_null, self.pve_se_null = nf["l_remle_null"], nf["pve"], nf["pve_se"]
        self.pheno_mean = float(pheno_mean)
        return self.l_remle_null

    def RidgeR(self, U, eval_, Uty, lambda_, geno, geno_kind, indicator_idv=None, ns_test=None, batch=LMM_BATCH_SIZE):
        """BSLMM::RidgeR (src/bslmm.cpp:1194-1221) without UtX: geno holds the SNP-major rows of the analysed SNPs (fp64 with NaN,
        or .bed bytes), over the analysed individuals or -- with indicator_idv -- over all of them.  ns_test: the SNP count the
        effects are scaled by (default: the rows of geno).  Returns (alpha, bv)."""
        n = U.shape[0]
        ns_test = geno.shape[0] if ns_test is None else ns_test
        U_c = _np64(np.ascontiguousarray(U), "U")
        ev_c = np.ascontiguousarray(eval_, dtype=np.float64)
        Uty_c = np.ascontiguousarray(Uty, dtype=np.float64)
        bv = np.zeros(n)
        L.check(L.lib().gemma_hip_ridge_setup(n, _ptr(U_c), _ptr(ev_c), _ptr(Uty_c), float(lambda_), int(ns_test), _ptr(bv)),
                "BSLMM.RidgeR")
        try:
            if indicator_idv is not None:
                ridge_set_indicator(indicator_idv)
            outs = [ridge_batch(blk, geno_kind) for blk in _blocks(geno, batch)]
        finally:
            ridge_finish()
        self.alpha = np.concatenate(outs) if outs else np.zeros(0)
        self.bv = bv
        return self.alpha, self.bv

    def WriteParam(self, path, snp_info, alpha=None):
        """BSLMM::WriteParam(alpha), src/bslmm.cpp:193-235: snp_info = dicts with chr, rs, ps, n_miss of the analysed SNPs."""
        alpha = self.alpha if alpha is None else alpha
        with open(path, "w") as f:
            f.write("chr\trs\tps\tn_miss\talpha\tbeta\tgamma\n")
            for si, a in zip(snp_info, alpha):
                # `scientific << setprecision(6)` stays set on the stream: the two zeros print in it too
                f.write("%s\t%s\t%s\t%d\t%.6e\t%.6e\t%.6e\n" % (si["chr"], si["rs"], si["ps"], si["n_miss"], a, 0.0, 0.0))

    def WriteBV(self, path, indicator_idv, bv=None):
        """BSLMM::WriteBV, src/bslmm.cpp:116-140"""
        bv = self.bv if bv is None else bv
        t = 0
        with open(path, "w") as f:
            for k in indicator_idv:
                if k == 0:
                    f.write("NA\n")
                else:
                    f.write("%.6e\n" % bv[t])
                    t += 1

    def WriteLog(self, path):
        """The lines of PARAM's log a later -predict run reads back (-emu; ReadFile_log, src/gemma_io.cpp:239-277) and the null
        fit's summary beside them, in the reference's wording and default precision (src/gemma.cpp:3300-3400)."""
        with open(path, "w") as f:
            f.write("##\n## Summary Statistics:\n")
            f.write("## pve estimate in the null model = %s\n" % _g6(self.pve_null))
            f.write("## se(pve) in the null model = %s\n" % _g6(self.pve_se_null))
            f.write("## estimated mean = %s\n" % _g6(self.pheno_mean))


def ReadFile_log(path):
    """ReadFile_log, src/gemma_io.cpp:239-277: the `estimated mean` of a -bslmm log (0 when the file has none)."""
    for line in open(path):
        t = line.replace(",", " ").split()
        if len(t) >= 5 and t[1] == "estimated" and t[2] == "mean" and t[3] == "=":
            return float(t[4])
    return 0.0


def ReadFile_est(path, est_column=None, have_ebv=False):
    """ReadFile_est, src/gemma_io.cpp:2224-2289, with the defaults of PARAM::CheckParam (src/param.cpp:671-684): columns
    rs, alpha, beta, gamma = 2 5 6 7, and 2 0 6 7 when an -ebv file is given -- column 0 is never met, so alpha stays 0 and a
    ridge `.param.txt` (beta = gamma = 0) then yields effects that are all zero.  effect = alpha + beta * gamma.
    Returns an ordered dict rs -> effect; a repeated SNP is an error, as in the reference."""
    if est_column is None:
        est_column = (2, 0, 6, 7) if have_ebv else (2, 5, 6, 7)
    n = max(est_column)
    out = {}
    with open(path) as f:
        f.readline()
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) < n:
                raise ValueError("%s: a row has %d columns, %d needed" % (path, len(t), n))
            alpha, beta, gamma = 0.0, 0.0, 1.0
            rs = t[est_column[0] - 1]
            if est_column[1] >= 1:
                alpha = float(t[est_column[1] - 1])
            if est_column[2] >= 1:
                beta = float(t[est_column[2] - 1])
            if est_column[3] >= 1:
                gamma = float(t[est_column[3] - 1])
            if rs in out:
                raise ValueError("the same SNP occurs more than once in estimated parameter file: %s" % rs)
            out[rs] = alpha + beta * gamma
    return out


class PRDT:
    """Mirror of class PRDT (src/prdt.h) for -predict 1 / 2 (a_mode 41 / 42), the block of src/gemma.cpp:1660-1729:

        p = PRDT(indicator_idv)            # 1 = phenotyped (training), 0 = to be predicted
        p.AddBV(G, u_hat)                  # optional: -ebv with -k
        p.AnalyzePlink(bed_rows, rs, mapRS2est)    # or AnalyzeBimbam(X, rs, mapRS2est)
        y = p.Finish(pheno_mean, a_mode)   # + mean, Phi() for a_mode 42
        p.WriteFiles(path, y)
    """

    def __init__(self, indicator_idv):
        self.indicator_idv = np.ascontiguousarray(indicator_idv, dtype=np.int32)
        self.ns_test = 0
        self.ignored = []
        L.check(L.lib().gemma_hip_prdt_begin(_ptr(self.indicator_idv), self.indicator_idv.size), "PRDT")

    def AddBV(self, G, u_hat):
        """PRDT::AddBV, src/prdt.cpp:133-205: G over all individuals (not changed), u_hat over the training individuals."""
        u = np.ascontiguousarray(u_hat, dtype=np.float64)
        ni = self.indicator_idv.size
        if _is_torch(G):
            rc = L.lib().gemma_hip_prdt_add_bv_d(C.c_void_p(G.data_ptr()), ni, _tld(G), _ptr(u), u.size, _stream())
        else:
            G_c = _np64(np.ascontiguousarray(G), "G")
            if G_c.shape != (ni, ni):
                raise ValueError("G must be %d x %d" % (ni, ni))
            rc = L.lib().gemma_hip_prdt_add_bv(_ptr(G_c), ni, _ptr(u), u.size)
        L.check(rc, "PRDT.AddBV")

    def _analyze(self, geno, geno_kind, rs, mapRS2est, batch):
        rs = list(rs)
        sel = np.array([i for i, r in enumerate(rs) if r in mapRS2est], dtype=np.int64)
        rows = np.ascontiguousarray(geno[sel])
        eff = np.array([mapRS2est[rs[i]] for i in sel], dtype=np.float64)
        self.ns_test = 0
        self.ignored = []
        for s0 in range(0, rows.shape[0], batch):
            blk = rows[s0:s0 + batch]
            w = np.ascontiguousarray(eff[s0:s0 + batch])
            used = np.zeros(blk.shape[0], dtype=np.int32)
            L.check(L.lib().gemma_hip_prdt_add(geno_kind, _ptr(blk), blk.shape[0], _row_ld(blk), _ptr(w),
                                               _ptr(used)), "PRDT.Analyze")
            self.ns_test += int(used.sum())
            self.ignored += [rs[sel[s0 + i]] for i in np.flatnonzero(used == 0)]

    def AnalyzePlink(self, bed_rows, rs, mapRS2est, batch=LMM_BATCH_SIZE):
        """PRDT::AnalyzePlink, src/prdt.cpp:310-444: bed_rows = the .bed payload (one row per SNP of the .bim, over all
        individuals), rs = their names; SNPs outside mapRS2est are passed over.  self.ignored: the SNPs missing in every
        individual to be predicted; self.ns_test: the SNPs used."""
        self._analyze(np.asarray(bed_rows, dtype=np.uint8), L.GENO_PLINK_2BIT, rs, mapRS2est, batch)

    def AnalyzeBimbam(self, X_snpmajor_nan, rs, mapRS2est, batch=LMM_BATCH_SIZE):
        """PRDT::AnalyzeBimbam, src/prdt.cpp:207-308: X over all individuals, NaN = NA."""
        self._analyze(np.asarray(X_snpmajor_nan, dtype=np.float64), L.GENO_F64_SNP_MAJOR, rs, mapRS2est, batch)

    def Finish(self, pheno_mean=0.0, a_mode=41):
        """src/gemma.cpp:1711-1722: + pheno_mean; a_mode 42 (-predict 2): Phi(y).  Ends the device state."""
        y = np.zeros(int((self.indicator_idv == 0).sum()))
        L.check(L.lib().gemma_hip_prdt_end(float(pheno_mean), 1 if a_mode == 42 else 0, _ptr(y)), "PRDT.Finish")
        return y

    @staticmethod
    def MvnormPrdt(G_full, indicator_pheno, W_full, y_full, l_min=1e-5, l_max=1e5, n_region=10):
        """-predict from a kinship alone (a_mode 43) for one phenotype: the block of src/gemma.cpp:1732-1820 / :1873-1882 around
        PRDT::MvnormPrdt (src/prdt.cpp:448-553).  G_full: the kinship of the individuals with covariates as it was read (not
        centred); indicator_pheno: 1 = observed; W_full with the intercept; y_full: entries of the unobserved ones are not read.
        Returns (Y_full with the missing entries predicted, dict(vg, ve, l_remle))."""
        ind = np.ascontiguousarray(indicator_pheno, dtype=np.int32)
        ni = ind.size
        G_c = _np64(np.ascontiguousarray(G_full), "G_full")
        W_c = np.ascontiguousarray(np.asarray(W_full, dtype=np.float64).reshape(ni, -1))
        y_c = np.ascontiguousarray(y_full, dtype=np.float64)
        if G_c.shape != (ni, ni) or y_c.shape != (ni,):
            raise ValueError("G_full must be %d x %d and y_full of length %d" % (ni, ni, ni))
        y_miss, fit = np.zeros(max(int((ind == 0).sum()), 1)), np.zeros(3)
        L.check(L.lib().gemma_hip_prdt_kin(ni, _ptr(G_c), _ptr(ind), _ptr(W_c), W_c.shape[1], _ptr(y_c), l_min, l_max, n_region,
                                           _ptr(y_miss), _ptr(fit)), "PRDT.MvnormPrdt")
        Y = y_c.copy()
        Y[ind == 0] = y_miss[:int((ind == 0).sum())]
        return Y, dict(vg=fit[0], ve=fit[1], l_remle=fit[2])

    @staticmethod
    def _mv_args(G_full, indicator_pheno, W_full, Y_full):
        ind = np.ascontiguousarray(indicator_pheno, dtype=np.int32)
        if ind.ndim != 2:
            raise ValueError("indicator_pheno must be ni x d")
        ni, d = ind.shape
        W_c = np.ascontiguousarray(np.asarray(W_full, dtype=np.float64).reshape(ni, -1))
        Y_c = np.ascontiguousarray(Y_full, dtype=np.float64)
        if Y_c.shape != (ni, d):
            raise ValueError("Y_full must be %d x %d" % (ni, d))
        if _is_torch(G_full):
            if tuple(G_full.shape) != (ni, ni):
                raise ValueError("G_full must be %d x %d" % (ni, ni))
            G_c = G_full
        else:
            G_c = _np64(np.ascontiguousarray(G_full), "G_full")
            if G_c.shape != (ni, ni):
                raise ValueError("G_full must be %d x %d" % (ni, ni))
        return ind, ni, d, G_c, W_c, Y_c, np.zeros(max(int((ind == 0).sum()), 1))

    @staticmethod
    def _mv_fill(Y_c, ind, y_miss):
        Y = Y_c.copy()
        Y[ind == 0] = y_miss[:int((ind == 0).sum())]  # boolean assignment runs in row-major order: i * d + a
        return Y

    @staticmethod
    def MvnormApply(G_full, indicator_pheno, W_full, Y_full, Vg, Ve, B):
        """The Kronecker system of a_mode 43 alone, for given Vg, Ve (d x d) and B (d x n_cvt): every unobserved (i, a) is
        predicted from the observed entries through H = Gc (x) Vg + I (x) Ve (the else branch of src/gemma.cpp:1821-1871 with
        PRDT::MvnormPrdt) without H_full.  G_full: numpy, or a torch tensor on the device (not changed).  Returns Y_full with the
        missing entries filled."""
        ind, ni, d, G_c, W_c, Y_c, y_miss = PRDT._mv_args(G_full, indicator_pheno, W_full, Y_full)
        c = W_c.shape[1]
        Vg_c, Ve_c = (np.ascontiguousarray(M, dtype=np.float64) for M in (Vg, Ve))
        B_c = np.ascontiguousarray(np.asarray(B, dtype=np.float64).reshape(d, -1))
        if Vg_c.shape != (d, d) or Ve_c.shape != (d, d) or B_c.shape != (d, c):
            raise ValueError("Vg, Ve must be %d x %d and B %d x %d" % (d, d, d, c))
        if _is_torch(G_c):
            rc = L.lib().gemma_hip_prdt_kin_mv_apply_d(ni, d, C.c_void_p(G_c.data_ptr()), _tld(G_c), _ptr(ind), _ptr(W_c), c, _ptr(Y_c),
                                                       _ptr(Vg_c), _ptr(Ve_c), _ptr(B_c), _ptr(y_miss), _stream())
        else:
            rc = L.lib().gemma_hip_prdt_kin_mv_apply(ni, d, _ptr(G_c), _ptr(ind), _ptr(W_c), c, _ptr(Y_c), _ptr(Vg_c), _ptr(Ve_c),
                                                     _ptr(B_c), _ptr(y_miss))
        L.check(rc, "PRDT.MvnormApply")
        return PRDT._mv_fill(Y_c, ind, y_miss)

    @staticmethod
    def MvnormPrdtMulti(G_full, indicator_pheno, W_full, Y_full, l_min=1e-5, l_max=1e5, n_region=10, em_iter=10000, nr_iter=100,
                        em_prec=1e-4, nr_prec=1e-4):
        """-predict from a kinship alone (a_mode 43) for several phenotypes, the whole block of src/gemma.cpp:1732-1897: the null
        model is fitted on the individuals with every trait (their kinship centred and decomposed, the REMLE fit of
        CalcMvLmmVgVeBeta), then every missing (individual, trait) entry is predicted.  indicator_pheno, Y_full: ni x d.
        Returns (Y_full with the missing entries filled, dict(Vg, Ve, B, logl_remle))."""
        ind, ni, d, G_c, W_c, Y_c, y_miss = PRDT._mv_args(G_full, indicator_pheno, W_full, Y_full)
        if _is_torch(G_c):
            raise TypeError("G_full must be a numpy array (MvnormApply takes a device matrix)")
        c = W_c.shape[1]
        opt, nf = L.MvOpt(em_iter, nr_iter, em_prec, nr_prec, 1e-3, 0, 0), L.MvNull()
        L.check(L.lib().gemma_hip_prdt_kin_mv(ni, d, _ptr(G_c), _ptr(ind), _ptr(W_c), c, _ptr(Y_c), l_min, l_max, n_region,
                                              C.byref(opt), _ptr(y_miss), C.byref(nf)), "PRDT.MvnormPrdtMulti")
        g = lambda a, r, k: np.array(a[:r * k]).reshape(r, k)
        return PRDT._mv_fill(Y_c, ind, y_miss), dict(Vg=g(nf.Vg_remle, d, d), Ve=g(nf.Ve_remle, d, d), B=g(nf.B_remle, d, c),
                                                     logl_remle=nf.logl_remle_H0)

    @staticmethod
    def WriteFilesFull(path, Y_full, indicator_cvt=None):
        """PRDT::WriteFiles(gsl_matrix *), src/prdt.cpp:104-131: one row per individual, NA without covariates, a tab after
        every value."""
        Y = np.asarray(Y_full, dtype=np.float64).reshape(len(Y_full), -1)
        ind = np.ones(Y.shape[0], dtype=np.int32) if indicator_cvt is None else np.asarray(indicator_cvt)
        t = 0
        with open(path, "w") as f:
            for k in ind:
                if k == 0:
                    f.write("NA\n")
                else:
                    f.write("".join(_g6(v) + "\t" for v in Y[t]) + "\n")
                    t += 1

    def WriteFiles(self, path, y_prdt):
        """PRDT::WriteFiles(gsl_vector *), src/prdt.cpp:76-102"""
        t = 0
        with open(path, "w") as f:
            for k in self.indicator_idv:
                if k == 1:
                    f.write("NA\n")
                else:
                    f.write(_g6(y_prdt[t]) + "\n")
                    t += 1


# ----------------------------------------------------------------------------- MQS summary statistics (-gs, -vc 1 -beta)
class MQS:
    """PARAM::CalcS (src/param.cpp:1717-1812) on the device, called where src/gemma.cpp:1977 (-gs) and :2166 (-vc 1 -beta) call it:

        m = MQS(indicator_idv, W, n_vc)        # W: ni_test x n_cvt with the intercept
        m.AnalyzePlink(bed_rows, cat, weight)  # rows of the SNPs with indicator_snp != 0; cat < 0: skipped; weight None: 1
        S, Svar, ns = m.Finish()               # prefix.S.txt = S on top of Svar, ns = the per-category SNP counts of size.txt
        K0 = m.Get(0, 0)                       # the centred + scaled kinship of category 0

    slot=1 fills A beside the K of a finished slot=0 pass (the second CalcS of src/gemma.cpp:2198); slot=2 does so on top of that
    K, which is what the reference's second CalcS computes (its PlinkKin adds to the A the first CalcS left)."""

    def __init__(self, indicator_idv, W, n_vc):
        self.indicator_idv = np.ascontiguousarray(indicator_idv, dtype=np.int32)
        self.n = int((self.indicator_idv != 0).sum())
        self.W = np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(self.n, -1))
        self.n_vc = int(n_vc)

    def _analyze(self, geno, geno_kind, cat, weight, slot, batch):
        lib = L.lib()
        L.check(lib.gemma_hip_mqs_begin(self.indicator_idv.size, _ptr(self.indicator_idv), self.n_vc, _ptr(self.W), self.W.shape[1],
                                        int(slot)), "MQS.begin")
        l = geno.shape[0]
        if _is_torch(geno):
            import torch
            cat_t = torch.as_tensor(np.asarray(cat, dtype=np.int32)).to(geno.device) if not _is_torch(cat) else cat
            w_t = None
            if weight is not None:
                w_t = torch.as_tensor(np.asarray(weight, dtype=np.float64)).to(geno.device) if not _is_torch(weight) else weight
            for s0 in range(0, l, batch):
                blk, cb = geno[s0:s0 + batch], cat_t[s0:s0 + batch]
                wp = C.c_void_p(w_t[s0:s0 + batch].data_ptr()) if w_t is not None else None
                L.check(lib.gemma_hip_mqs_add_d(geno_kind, C.c_void_p(blk.data_ptr()), blk.shape[0], _tld(geno), C.c_void_p(cb.data_ptr()),
                                                wp, _stream()), "MQS.add")
            return
        cat = np.ascontiguousarray(cat, dtype=np.int32)
        weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        if cat.shape != (l,) or (weight is not None and weight.shape != (l,)):
            raise ValueError("cat and weight take one entry per SNP row")
        geno = np.ascontiguousarray(geno)
        for s0 in range(0, l, batch):
            blk, cb = geno[s0:s0 + batch], cat[s0:s0 + batch]
            wb = None if weight is None else weight[s0:s0 + batch]
            L.check(lib.gemma_hip_mqs_add(geno_kind, _ptr(blk), blk.shape[0], _row_ld(blk), _ptr(cb),
                                          None if wb is None else _ptr(wb)), "MQS.add")

    def AnalyzePlink(self, bed_rows, cat, weight=None, slot=0, batch=K_BATCH_SIZE):
        """PlinkKin with weights and categories, src/gemma_io.cpp:2947-3170: bed_rows = .bed rows over all ni_total individuals."""
        if not _is_torch(bed_rows):
            bed_rows = np.asarray(bed_rows, dtype=np.uint8)
        self._analyze(bed_rows, L.GENO_PLINK_2BIT, cat, weight, slot, batch)

    def AnalyzeBimbam(self, G, cat, weight=None, slot=0, batch=K_BATCH_SIZE):
        """BimbamKinUncentered, src/gemma_io.cpp:2753-2945: G SNP-major over all individuals, NaN = NA."""
        if not _is_torch(G):
            G = np.asarray(G, dtype=np.float64)
        self._analyze(G, L.GENO_F64_SNP_MAJOR, cat, weight, slot, batch)

    def Finish(self):
        S = np.zeros((2 * self.n_vc, self.n_vc))
        ns = np.zeros(self.n_vc)
        L.check(L.lib().gemma_hip_mqs_end(_ptr(S), _ptr(ns)), "MQS.Finish")
        return S[:self.n_vc].copy(), S[self.n_vc:].copy(), ns

    def Get(self, slot, i):
        out = np.zeros((self.n, self.n))
        L.check(L.lib().gemma_hip_mqs_get(int(slot), int(i), _ptr(out)), "MQS.Get")
        return out

    @staticmethod
    def S(A, K, n_cvt):
        """gemma_hip_mqs_S: (S, Svar) from centred + scaled matrices A, K of shape (n_vc, n, n); `A is K` halves the work."""
        K_c = _np64(np.ascontiguousarray(K), "K")
        A_c = K_c if A is K else _np64(np.ascontiguousarray(A), "A")
        n_vc, n = K_c.shape[0], K_c.shape[1]
        if K_c.shape != (n_vc, n, n) or A_c.shape != K_c.shape:
            raise ValueError("A and K must be n_vc x n x n")
        S = np.zeros((2 * n_vc, n_vc))
        L.check(L.lib().gemma_hip_mqs_S(n, n_vc, _ptr(A_c), _ptr(K_c), n, int(n_cvt), _ptr(S)), "MQS.S")
        return S[:n_vc].copy(), S[n_vc:].copy()

    @staticmethod
    def Release():
        L.check(L.lib().gemma_hip_mqs_release(), "MQS.Release")


# ----------------------------------------------------------------------------- MQS confidence intervals (-ci 1, -ci 2)
class CI:
    """The two genotype passes of the MQS confidence intervals on the device, called where src/gemma.cpp:2400-2554 calls PlinkXwz /
    BimbamXwz and PlinkXtXwz / BimbamXtXwz (src/vc.cpp:2225-2437, :2480-2688):

        ci = CI(indicator_idv, n_vc)
        Xz, XWz, XtXWz, n_skipped = ci.AnalyzePlink(bed_rows, cat, z, w)   # rows of the analysed SNPs in file order; w None: -ci 1

    Xz, XWz: ni_test x n_vc; XtXWz: one row per SNP row; n_skipped: SNPs without a called genotype or without variance among the
    analysed individuals (zero rows of XtXWz; the reference divides by 0 there)."""

    def __init__(self, indicator_idv, n_vc):
        self.indicator_idv = np.ascontiguousarray(indicator_idv, dtype=np.int32)
        self.n = int((self.indicator_idv != 0).sum())
        self.n_vc = int(n_vc)

    def _analyze(self, geno, geno_kind, cat, z, w, batch):
        lib = L.lib()
        l, n_vc = geno.shape[0], self.n_vc
        dev = _is_torch(geno)
        L.check(lib.gemma_hip_ci_begin(self.indicator_idv.size, _ptr(self.indicator_idv), n_vc), "CI.begin")
        Xz, XWz = np.zeros((self.n, n_vc)), np.zeros((self.n, n_vc))
        n_skipped, skipped = 0, C.c_size_t(0)
        if dev:
            import torch

            def _t(v, dt, name):
                if not _is_torch(v):
                    return torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).to(geno.device)
                want = torch.int32 if dt is np.int32 else torch.float64
                if v.dtype != want or v.device != geno.device or not v.is_contiguous() or tuple(v.shape) != (l,):
                    raise ValueError("%s: a contiguous %s tensor with one entry per SNP row on the device of the rows" % (name, want))
                return v
            if not geno.is_contiguous():
                raise ValueError("the genotype rows must be contiguous")
            cat_t, z_t = _t(cat, np.int32, "cat"), _t(z, np.float64, "z")
            w_t = None if w is None else _t(w, np.float64, "w")
            out = torch.zeros((l, n_vc), dtype=torch.float64, device=geno.device)
        else:
            geno = np.ascontiguousarray(geno)
            cat, z = np.ascontiguousarray(cat, dtype=np.int32), np.ascontiguousarray(z, dtype=np.float64)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
            if cat.shape != (l,) or z.shape != (l,) or (w is not None and w.shape != (l,)):
                raise ValueError("cat, z and w take one entry per SNP row")
            out = np.zeros((l, n_vc))
        for s0 in range(0, l, batch):  # pass 1
            blk = geno[s0:s0 + batch]
            if dev:
                wp = C.c_void_p(w_t[s0:s0 + batch].data_ptr()) if w_t is not None else None
                L.check(lib.gemma_hip_ci_xwz_d(geno_kind, C.c_void_p(blk.data_ptr()), blk.shape[0], _tld(geno),
                                               C.c_void_p(cat_t[s0:s0 + batch].data_ptr()), C.c_void_p(z_t[s0:s0 + batch].data_ptr()), wp,
                                               C.byref(skipped), _stream()), "CI.xwz")
            else:
                L.check(lib.gemma_hip_ci_xwz(geno_kind, _ptr(blk), blk.shape[0], _row_ld(blk), _ptr(cat[s0:s0 + batch]),
                                             _ptr(z[s0:s0 + batch]), None if w is None else _ptr(w[s0:s0 + batch]), C.byref(skipped)),
                        "CI.xwz")
            n_skipped += skipped.value
        L.check(lib.gemma_hip_ci_xwz_end(_ptr(Xz), _ptr(XWz)), "CI.xwz_end")
        for s0 in range(0, l, batch):  # pass 2
            blk, ob = geno[s0:s0 + batch], out[s0:s0 + batch]
            if dev:
                L.check(lib.gemma_hip_ci_xtxwz_d(geno_kind, C.c_void_p(blk.data_ptr()), blk.shape[0], _tld(geno),
                                                 C.c_void_p(ob.data_ptr()), _stream()), "CI.xtxwz")
            else:
                L.check(lib.gemma_hip_ci_xtxwz(geno_kind, _ptr(blk), blk.shape[0], _row_ld(blk), _ptr(ob)), "CI.xtxwz")
        if dev:
            import torch
            torch.cuda.synchronize()
        return Xz, XWz, out, n_skipped

    def AnalyzePlink(self, bed_rows, cat, z, w=None, batch=LMM_BATCH_SIZE):
        """PlinkXwz then PlinkXtXwz, src/vc.cpp:2314-2437, :2568-2688: bed_rows = .bed rows over all ni_total individuals."""
        if not _is_torch(bed_rows):
            bed_rows = np.asarray(bed_rows, dtype=np.uint8)
        return self._analyze(bed_rows, L.GENO_PLINK_2BIT, cat, z, w, batch)

    def AnalyzeBimbam(self, G, cat, z, w=None, batch=LMM_BATCH_SIZE):
        """BimbamXwz then BimbamXtXwz, src/vc.cpp:2225-2312, :2480-2566: G SNP-major over all individuals, NaN = NA.  The
        individuals are the ones indicator_idv selects (the reference takes the first ni_test tokens of a line)."""
        if not _is_torch(G):
            G = np.asarray(G, dtype=np.float64)
        return self._analyze(G, L.GENO_F64_SNP_MAJOR, cat, z, w, batch)

    @staticmethod
    def Release():
        L.check(L.lib().gemma_hip_ci_release(), "CI.Release")


# ----------------------------------------------------------------------------- windowed SNP correlation (-calccor)
def _sci6(v):
    """`scientific << setprecision(6)` of an ostream"""
    v = float(v)
    if v != v:
        return "-nan" if np.signbit(v) else "nan"
    return "%.6e" % v


class VARCOV:
    """VARCOV (src/varcov.cpp) on the device, called where src/gemma.cpp:2046-2059 calls it (-calccor, a_mode 71):

        v = VARCOV(indicator_idv, indicator_snp, chr, cM, bp, window_bp=300)   # chr / cM / bp of ALL SNPs, as snpInfo holds them
        n_nb = v.CalcNB()                        # per SNP (0 where indicator_snp == 0)
        var, cor, off = v.AnalyzePlink(bed_rows) # rows of the SNPs with indicator_snp != 0, in file order
        v.WriteCov(path, snpinfo)                # prefix.cor.txt

    var[j], cor[off[j]:off[j + 1]] belong to analysed SNP j.  The window of a SNP is exactly CalcNB's n_nb (the
    reference's sliding buffer can carry leftover rows on input that is not sorted by position; on sorted input the two agree)."""

    def __init__(self, indicator_idv, indicator_snp, chr, cM, bp, window_cm=0, window_bp=0, window_ns=0):
        self.indicator_idv = np.ascontiguousarray(indicator_idv, dtype=np.int32)
        self.indicator_snp = np.ascontiguousarray(indicator_snp, dtype=np.int32)
        self.chr = [str(c) for c in chr]
        self.cM = np.asarray(cM, dtype=np.float64)
        self.bp = np.asarray(bp, dtype=np.int64)
        ns = self.indicator_snp.size
        if len(self.chr) != ns or self.cM.shape != (ns,) or self.bp.shape != (ns,):
            raise ValueError("chr, cM and bp take one entry per SNP of indicator_snp")
        self.window_cm, self.window_bp, self.window_ns = float(window_cm), int(window_bp), int(window_ns)
        if self.window_cm == 0 and self.window_bp == 0 and self.window_ns == 0:
            self.window_bp = 1000000  # src/param.cpp:629-630
        self.ni_test = int((self.indicator_idv != 0).sum())
        self.n_nb = None
        self.var = self.cor = self.off = None

    def CalcNB(self):
        """VARCOV::CalcNB, src/varcov.cpp:168-217, branch for branch"""
        ind, chr_, cM, bp = self.indicator_snp, self.chr, self.cM, self.bp
        ns = ind.size
        w_cm, w_bp, w_ns = self.window_cm, self.window_bp, self.window_ns
        out = np.zeros(ns, dtype=np.int32)
        for t in range(ns):
            if ind[t] == 0:
                continue
            if chr_[t] == "-9" or (cM[t] == -9 and w_cm != 0) or (bp[t] == -9 and w_bp != 0):
                continue
            if t == ns - 1:
                continue
            t2, n_nb = t + 1, 0
            while t2 < ns and chr_[t2] == chr_[t] and ind[t2] == 0:
                t2 += 1
            while (t2 < ns and chr_[t2] == chr_[t] and (cM[t2] - cM[t] < w_cm or w_cm == 0) and
                   (bp[t2] - bp[t] < w_bp or w_bp == 0) and (n_nb < w_ns or w_ns == 0)):
                t2 += 1
                n_nb += 1
                while t2 < ns and chr_[t2] == chr_[t] and ind[t2] == 0:
                    t2 += 1
            out[t] = n_nb
        self.n_nb = out
        return out

    def _analyze(self, geno, geno_kind, batch):
        if self.n_nb is None:
            self.CalcNB()
        nb = np.ascontiguousarray(self.n_nb[self.indicator_snp != 0])  # analysed SNPs only: the rows of geno
        l = nb.size
        if geno.shape[0] != l:
            raise ValueError("geno holds %d rows, indicator_snp keeps %d SNPs" % (geno.shape[0], l))
        off = np.zeros(l + 1, dtype=np.int64)
        np.cumsum(nb, out=off[1:])
        lib = L.lib()
        L.check(lib.gemma_hip_cor_begin(self.indicator_idv.size, _ptr(self.indicator_idv)), "VARCOV.begin")
        dev = _is_torch(geno)
        if dev:
            import torch
            var = torch.empty(l, dtype=torch.float64, device=geno.device)
            cor = torch.empty(max(int(off[-1]), 1), dtype=torch.float64, device=geno.device)
            nb_t = torch.as_tensor(nb).to(geno.device)
        else:
            geno = np.ascontiguousarray(geno)
            var, cor = np.zeros(l), np.zeros(max(int(off[-1]), 1))
        for s0 in range(0, l, batch):  # batch outputs and the halo their windows reach into (re-read with the next block)
            s1 = min(l, s0 + batch)
            l_in = int(max(s1, (np.arange(s0, s1) + nb[s0:s1]).max() + 1)) - s0
            blk = geno[s0:s0 + l_in]
            if dev:
                L.check(lib.gemma_hip_cor_block_d(geno_kind, C.c_void_p(blk.data_ptr()), l_in, _tld(geno), s1 - s0,
                                                  C.c_void_p(nb_t[s0:s1].data_ptr()), C.c_void_p(var[s0:s1].data_ptr()),
                                                  C.c_void_p(cor[int(off[s0]):].data_ptr()), _stream()), "VARCOV.block")
            else:
                L.check(lib.gemma_hip_cor_block(geno_kind, _ptr(blk), l_in, _row_ld(blk), s1 - s0, _ptr(nb[s0:s1]),
                                                _ptr(var[s0:s1]), _ptr(cor[int(off[s0]):])), "VARCOV.block")
        if dev:
            import torch
            torch.cuda.synchronize()
        self.var, self.cor, self.off = var, cor[:int(off[-1])], off
        return self.var, self.cor, self.off

    def AnalyzePlink(self, bed_rows, batch=LMM_BATCH_SIZE):
        """VARCOV::AnalyzePlink, src/varcov.cpp:348-446: bed_rows = .bed rows over all ni_total individuals."""
        if not _is_torch(bed_rows):
            bed_rows = np.asarray(bed_rows, dtype=np.uint8)
        return self._analyze(bed_rows, L.GENO_PLINK_2BIT, batch)

    def AnalyzeBimbam(self, G, batch=LMM_BATCH_SIZE):
        """VARCOV::AnalyzeBimbam, src/varcov.cpp:249-346: G SNP-major over all individuals, NaN = NA."""
        if not _is_torch(G):
            G = np.asarray(G, dtype=np.float64)
        return self._analyze(G, L.GENO_F64_SNP_MAJOR, batch)

    def WriteCov(self, path, snpinfo, var=None, cor=None, off=None):
        """VARCOV::WriteCov, src/varcov.cpp:74-145.  snpinfo: one (chr, rs, ps, n_miss, n_idv, a_minor, a_major, maf) per analysed
        SNP; var / cor / off default to the last Analyze* call."""
        var = self.var if var is None else var
        cor = self.cor if cor is None else cor
        off = self.off if off is None else off
        if _is_torch(var):
            var, cor = var.cpu().numpy(), cor.cpu().numpy()
        with open(path, "w") as f:
            f.write("chr\trs\tps\tn_mis\tn_obs\tallele1\tallele0\taf\twindow_size\tvar\tcor\n")
            for j, (chr_, rs, ps, n_miss, n_idv, a1, a0, maf) in enumerate(snpinfo):
                w = int(off[j + 1] - off[j])
                f.write("%s\t%s\t%d\t%d\t%d\t%s\t%s\t%.3f\t%d\t%s\t" % (chr_, rs, ps, n_miss, n_idv, a1, a0, maf, w, _sci6(var[j])))
                f.write(",".join(_sci6(v) for v in cor[off[j]:off[j + 1]]) if w else "NA")
                f.write("\n")

    @staticmethod
    def Release():
        L.check(L.lib().gemma_hip_cor_release(), "VARCOV.Release")


_HEADER_SETS = dict(  # ReadHeader_io, src/gemma_io.cpp:2367-2427 (the a1 / a0 sets as the reference builds them: one name short each)
    rs=("rs", "RS", "snp", "SNP", "snps", "SNPS", "snpid", "SNPID", "rsid", "RSID", "MarkerName"),
    chr=("chr", "CHR"), pos=("ps", "PS", "pos", "POS", "base_position", "BASE_POSITION", "bp", "BP"), cm=("cm", "CM"),
    a1=("a1", "A1", "allele1", "ALLELE1", "Allele1"),
    a0=("a0", "A0", "allele0", "ALLELE0", "Allele0", "a2", "A2", "allele2", "ALLELE2", "Allele2"),
    z=("z", "Z", "z_score", "Z_SCORE", "zscore", "ZSCORE"), beta=("beta", "BETA", "b", "B"),
    sebeta=("se_beta", "SE_BETA", "se", "SE"), chisq=("chisq", "CHISQ", "chisquare", "CHISQUARE"),
    p=("p", "P", "pvalue", "PVALUE", "p-value", "P-VALUE"), n=("n", "N", "ntotal", "NTOTAL", "n_total", "N_TOTAL"),
    nmis=("nmis", "NMIS", "n_mis", "N_MIS", "n_miss", "N_MISS"), nobs=("nobs", "NOBS", "n_obs", "N_OBS"),
    ncase=("ncase", "NCASE", "n_case", "N_CASE"), ncontrol=("ncontrol", "NCONTROL", "n_control", "N_CONTROL"),
    ws=("window_size", "WINDOW_SIZE", "ws", "WS"),
    af=("af", "AF", "maf", "MAF", "f", "F", "allele_freq", "ALLELE_FREQ", "allele_frequency", "ALLELE_FREQUENCY",
        "Freq.Allele1.HapMapCEU", "FreqAllele1HapMapCEU", "Freq1.Hapmap"),
    cor=("cor", "COR", "r", "R"))
_HEADER_ORDER = ("rs", "chr", "pos", "cm", "a1", "a0", "z", "beta", "sebeta", "chisq", "p", "n", "nmis", "nobs", "ncase", "ncontrol",
                 "ws", "af", "cor")


def _tokens(line):
    return [t for t in line.replace(",", " ").replace("\t", " ").split(" ") if t]


def _open_text(path):
    import gzip
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rt") if gz else open(path, "r")


def ReadHeader_io(line):
    """src/gemma_io.cpp:2367-2629: column numbers (1-based, 0 = absent) by header name; every other column is a category."""
    h = {k + "_col": 0 for k in _HEADER_ORDER}
    h["cat_cols"] = []
    coln = 0
    for tok in _tokens(line):
        for k in _HEADER_ORDER:
            if tok in _HEADER_SETS[k]:
                if h[k + "_col"] == 0:
                    h[k + "_col"] = coln + 1
                break
        else:
            h["cat_cols"].append(coln + 1)
        coln += 1
    h["coln"] = coln
    return h


def _atoi(tok):
    import re
    m = re.match(r"\s*[+-]?\d+", tok)
    return int(m.group(0)) if m else 0


def _atof(tok):
    import re
    m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|nan|inf(inity)?)", tok, re.I)
    return float(m.group(0)) if m else 0.0


def ReadFile_cat(file_cat):
    """src/gemma_io.cpp:2634-2718 -> (mapRS2cat, n_vc): the first category column holding 1 names the SNP's category; a SNP with
    0 in every column is in no category."""
    mapRS2cat = {}
    with _open_text(file_cat) as f:
        lines = f.read().splitlines()
    h = ReadHeader_io(lines[0])
    named = ("rs", "chr", "pos", "cm", "a1", "a0")
    n_vc = h["coln"] - sum(1 for k in named if h[k + "_col"] != 0)
    rs = chr_ = pos = ""
    for line in lines[1:]:
        toks = _tokens(line)
        if not toks:
            continue
        i_cat = 0
        for i in range(h["coln"]):
            tok = toks[i]
            if h["rs_col"] == i + 1:
                rs = tok
            elif h["chr_col"] == i + 1:
                chr_ = tok
            elif h["pos_col"] == i + 1:
                pos = tok
            elif i + 1 in (h["cm_col"], h["a1_col"], h["a0_col"]):
                pass
            elif _atoi(tok) in (0, 1):
                if i_cat == 0 and h["rs_col"] == 0:
                    rs = chr_ + ":" + pos
                if _atoi(tok) == 1 and rs not in mapRS2cat:
                    mapRS2cat[rs] = i_cat
                i_cat += 1
    return mapRS2cat, n_vc


def _norm_ppf(p):
    """Inverse of the standard normal distribution function (Acklam's rational approximation, one Halley step on erfc)."""
    import math
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01,
         2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00,
         2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    if p <= 0.0:
        return -math.inf
    if p >= 1.0:
        return math.inf
    if p < 0.02425:
        q = math.sqrt(-2 * math.log(p))
        x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1)
    elif p > 1 - 0.02425:
        q = math.sqrt(-2 * math.log(1 - p))
        x = -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1)
    else:
        q = p - 0.5
        r = q * q
        x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1)
    e = 0.5 * math.erfc(-x / math.sqrt(2)) - p
    u = e * math.sqrt(2 * math.pi) * math.exp(x * x / 2)
    return x - u / (1 + x * u / 2)


def ReadFile_beta(file_beta, mapRS2cat, mapRS2wA):
    """The z-score overload of ReadFile_beta, src/gemma_io.cpp:3363-3551 -> dict(vec_cat, vec_ni, vec_weight, vec_z2, ni_total,
    ns_total, ns_test).  z from z, else beta / se, else chisq, else the p-value (gsl_cdf_chisq_Qinv(p, 1))."""
    vec_cat, vec_ni, vec_weight, vec_z2 = [], [], [], []
    ni_total = ns_total = ns_test = 0
    with _open_text(file_beta) as f:
        lines = f.read().splitlines()
    h = ReadHeader_io(lines[0])
    rs = chr_ = pos = ""
    for line in lines[1:]:
        if not line.strip(" \t\r"):
            continue
        toks = _tokens(line)
        z = beta = se = chisq = pv = 0.0
        n_total = n_mis = n_obs = n_case = n_control = 0
        for i in range(h["coln"]):
            tok, k = toks[i], i + 1
            if h["rs_col"] == k:
                rs = tok
            if h["chr_col"] == k:
                chr_ = tok
            if h["pos_col"] == k:
                pos = tok
            if h["z_col"] == k:
                z = _atof(tok)
            if h["beta_col"] == k:
                beta = _atof(tok)
            if h["sebeta_col"] == k:
                se = _atof(tok)
            if h["chisq_col"] == k:
                chisq = _atof(tok)
            if h["p_col"] == k:
                pv = _atof(tok)
            if h["n_col"] == k:
                n_total = _atoi(tok)
            if h["nmis_col"] == k:
                n_mis = _atoi(tok)
            if h["nobs_col"] == k:
                n_obs = _atoi(tok)
            if h["ncase_col"] == k:
                n_case = _atoi(tok)
            if h["ncontrol_col"] == k:
                n_control = _atoi(tok)
        if h["rs_col"] == 0:
            rs = chr_ + ":" + pos
        if h["n_col"] == 0:
            n_total = n_mis + n_obs if (h["nmis_col"] != 0 and h["nobs_col"] != 0) else n_case + n_control
        if h["z_col"] != 0:
            z2 = z * z
        elif h["beta_col"] != 0 and h["sebeta_col"] != 0:
            z = beta / se if se != 0 else (float("nan") if beta == 0 else float("inf"))
            z2 = z * z
        elif h["chisq_col"] != 0:
            z2 = chisq
        elif h["p_col"] != 0:
            z2 = _norm_ppf(pv / 2) ** 2
        else:
            z2 = 0.0
        if (not mapRS2wA or rs in mapRS2wA) and (not mapRS2cat or rs in mapRS2cat) and z2 != 0:
            vec_cat.append(mapRS2cat[rs] if mapRS2cat else 0)
            vec_ni.append(n_total)
            vec_weight.append(mapRS2wA[rs] if mapRS2wA else 1.0)
            vec_z2.append(z2)
            ni_total = max(ni_total, n_total)
            ns_test += 1
        ns_total += 1
    return dict(vec_cat=np.array(vec_cat, dtype=np.int64), vec_ni=np.array(vec_ni, dtype=np.int64),
                vec_weight=np.array(vec_weight, dtype=np.float64), vec_z2=np.array(vec_z2, dtype=np.float64),
                ni_total=ni_total, ns_total=ns_total, ns_test=ns_test)


def ObtainWeight(rs_analysed, setSnps_beta, mapRS2cat, mapRS2wcat=None):
    """PARAM::ObtainWeight without -wsnp, src/param.cpp:2214-2296: weight 1 for every analysed SNP that is in the beta file (when
    one is given), in the -wcat file (when one is given, :2235) and in a category (when categories are given)."""
    return {rs: 1.0 for rs in rs_analysed if (not setSnps_beta or rs in setSnps_beta) and (not mapRS2wcat or rs in mapRS2wcat) and
            (not mapRS2cat or rs in mapRS2cat)}


def ReadFile_wcat(file_wcat, n_vc):
    """The -wcat overload of ReadFile_wsnp, src/gemma_io.cpp:3281-3353 -> mapRS2wcat: per SNP its n_vc weights, one per column
    that is not rs / chr / pos / cm / a1 / a0."""
    mapRS2wcat = {}
    with _open_text(file_wcat) as f:
        lines = f.read().splitlines()
    h = ReadHeader_io(lines[0])
    rs = chr_ = pos = ""
    for line in lines[1:]:
        if not line.strip(" \t\r"):
            continue
        toks = _tokens(line)
        weight = []
        for i in range(h["coln"]):
            tok, k = toks[i], i + 1
            if h["rs_col"] == k:
                rs = tok
            elif h["chr_col"] == k:
                chr_ = tok
            elif h["pos_col"] == k:
                pos = tok
            elif k in (h["cm_col"], h["a1_col"], h["a0_col"]):
                pass
            else:
                weight.append(_atof(tok))
        if len(weight) != n_vc:
            raise ValueError("Number of columns in the wcat file does not match that of cat file.")
        if h["rs_col"] == 0:
            rs = chr_ + ":" + pos
        mapRS2wcat[rs] = weight
    return mapRS2wcat


def UpdateWeight(pve_flag, mapRS2wK, ni_test, ns, v_pve, mapRS2wcat, mapRS2cat):
    """PARAM::UpdateWeight, src/param.cpp:2300-2349 -> mapRS2wA: 1 / (1 + sum_i ni_test / ns_i wcat_i pve_i)^2 per SNP of mapRS2wK
    (in the map's order), normalised to mean 1 within each category.  pve_flag 1 clamps pve to [0, 1] (-vc 2), 0 does not (-ci 2)."""
    n_vc = len(v_pve)
    wsum, wcount = [0.0] * n_vc, [0.0] * n_vc
    mapRS2wA = {}
    for rs in sorted(mapRS2wK):
        wc = mapRS2wcat.get(rs, [0.0] * n_vc)
        d = 1.0
        for i in range(n_vc):
            if v_pve[i] >= 1 and pve_flag == 1:
                d += float(ni_test) / float(ns[i]) * wc[i]
            elif v_pve[i] <= 0 and pve_flag == 1:
                d += 0
            else:
                d += float(ni_test) / float(ns[i]) * wc[i] * float(v_pve[i])
        mapRS2wA[rs] = 1 / (d * d)
        k = mapRS2cat[rs] if mapRS2cat else 0
        wsum[k] += mapRS2wA[rs]
        wcount[k] += 1
    for i in range(n_vc):
        wsum[i] = wsum[i] / wcount[i] if wcount[i] != 0 else float("nan")
    for rs in mapRS2wA:
        mapRS2wA[rs] /= wsum[mapRS2cat[rs] if mapRS2cat else 0]
    return mapRS2wA


def ReadFile_beta_z(file_beta, mapRS2wA):
    """The (mapRS2wA, mapRS2A1, mapRS2z) overload of ReadFile_beta, src/gemma_io.cpp:3553-3714 -> (mapRS2A1, mapRS2z): the signed z
    (from z, else beta / se, else 0) and the allele it refers to.  Without an allele column a1 stays the empty string."""
    mapRS2A1, mapRS2z = {}, {}
    with _open_text(file_beta) as f:
        lines = f.read().splitlines()
    h = ReadHeader_io(lines[0])
    rs = chr_ = pos = a1 = ""
    for line in lines[1:]:
        if not line.strip(" \t\r"):
            continue
        toks = _tokens(line)
        z = beta = se = 0.0
        for i in range(h["coln"]):
            tok, k = toks[i], i + 1
            if h["rs_col"] == k:
                rs = tok
            if h["chr_col"] == k:
                chr_ = tok
            if h["pos_col"] == k:
                pos = tok
            if h["a1_col"] == k:
                a1 = tok
            if h["z_col"] == k:
                z = _atof(tok)
            if h["beta_col"] == k:
                beta = _atof(tok)
            if h["sebeta_col"] == k:
                se = _atof(tok)
        if h["rs_col"] == 0:
            rs = chr_ + ":" + pos
        if h["z_col"] != 0:
            pass
        elif h["beta_col"] != 0 and h["sebeta_col"] != 0:
            z = beta / se if se != 0 else (float("nan") if beta == 0 else float("inf"))
        else:
            z = 0.0
        if not mapRS2wA or rs in mapRS2wA:
            mapRS2z[rs] = z
            mapRS2A1[rs] = a1
    return mapRS2A1, mapRS2z


def UpdateSNPnZ(rs_analysed, a_minor, mapRS2wA, mapRS2A1, mapRS2z, mapRS2cat):
    """PARAM::UpdateSNPnZ, src/param.cpp:2353-2416 (one genotype file) -> (keep, w, z, vec_cat): keep[t] says whether analysed SNP t
    stays in indicator_snp (it has a weight); w, z, vec_cat run over the kept SNPs in file order.  z is negated when the beta
    file's allele differs from the genotype file's minor allele -- for every SNP when the beta file names no allele."""
    keep, w, z, vec_cat = [], [], [], []
    for rs, a1 in zip(rs_analysed, a_minor):
        if rs in mapRS2wA:
            z.append(mapRS2z[rs] if a1 == mapRS2A1[rs] else -1 * mapRS2z[rs])
            vec_cat.append(mapRS2cat[rs] if mapRS2cat else 0)
            w.append(mapRS2wA[rs])
            keep.append(True)
        else:
            keep.append(False)
    return np.array(keep, dtype=bool), np.array(w, dtype=np.float64), np.array(z, dtype=np.float64), np.array(vec_cat, dtype=np.int32)


def _read_numbers(path):
    with _open_text(path) as f:
        return [[_atof(t) for t in _tokens(line)] for line in f.read().splitlines() if line.strip(" \t\r")]


def ReadFile_ref(file_ref):
    """src/gemma_io.cpp:3987-4009 -> (S, Svar, s_vec, ni): prefix.S.txt (S on top of Svar) and prefix.size.txt (ns per category,
    then the number of individuals)."""
    size = [r[0] for r in _read_numbers(file_ref + ".size.txt")]
    n_vc = len(size) - 1
    M = np.array(_read_numbers(file_ref + ".S.txt"), dtype=np.float64)
    if M.shape != (2 * n_vc, n_vc):
        raise ValueError("%s.S.txt is %s, %s.size.txt names %d categories" % (file_ref, M.shape, file_ref, n_vc))
    return M[:n_vc].copy(), M[n_vc:].copy(), np.array(size[:n_vc]), int(size[n_vc])


def ReadFile_study(file_study):
    """src/gemma_io.cpp:3961-3985 -> (Vq, q, s_vec, ni): prefix.Vq.txt, prefix.q.txt and prefix.size.txt."""
    size = [r[0] for r in _read_numbers(file_study + ".size.txt")]
    n_vc = len(size) - 1
    Vq = np.array(_read_numbers(file_study + ".Vq.txt"), dtype=np.float64).reshape(n_vc, n_vc)
    q = np.array([r[0] for r in _read_numbers(file_study + ".q.txt")], dtype=np.float64)
    return Vq, q, np.array(size[:n_vc]), int(size[n_vc])


def CalcVCss_study(file_study, file_ref):
    """-study PREFIX -ref PREFIX without genotypes, src/gemma.cpp:2231-2330: ReadFile_study + ReadFile_ref + CalcVCss with the
    study's SNP counts and sample size (:2299).  The reference panel's counts and ni_ref only go into the size vector the run
    writes (:2305-2307): the `size` entry of the result."""
    Vq, q, s_study, ni_study = ReadFile_study(file_study)
    S, Svar, s_ref, ni_ref = ReadFile_ref(file_ref)
    if len(s_study) != len(s_ref):
        raise ValueError("%s names %d categories, %s names %d" % (file_study, len(s_study), file_ref, len(s_ref)))
    est = CalcVCss(Vq, S, Svar, q, s_study, ni_study)
    est["size"] = np.append(s_ref, float(ni_ref))
    return est


def CalcCIss(Xz, XWz, XtXWz, S_mat, Svar_mat, w, z, s_vec, vec_cat, v_pve):
    """src/vc.cpp:2727-2950 -> dict(pve, se_pve, pve_total, se_pve_total, sigma2, se_sigma2, enrich, se_enrich): the standard errors
    of given pve from the two genotype passes (class CI), S and Svar of the reference panel (ReadFile_ref), w / z / vec_cat of
    UpdateSNPnZ and s_vec = the number of SNPs per category.  O(p n_vc^2 + n n_vc^2) on the host."""
    Xz, XWz, XtXWz = (np.asarray(a, dtype=np.float64) for a in (Xz, XWz, XtXWz))
    S_mat, Svar_mat = np.asarray(S_mat, dtype=np.float64), np.asarray(Svar_mat, dtype=np.float64)
    w, z, s_vec, v_pve = (np.asarray(a, dtype=np.float64) for a in (w, z, s_vec, v_pve))
    vec_cat = np.asarray(vec_cat, dtype=np.int64)
    ni_test, n_vc = XWz.shape
    zwz, zz = np.zeros(n_vc), np.zeros(n_vc)
    np.add.at(zwz, vec_cat, w * z * z)
    np.add.at(zz, vec_cat, z * z)
    s_pve, s_snp = float(v_pve.sum()), float(s_vec.sum())
    Xz_pve = Xz @ (v_pve / s_vec)
    w_pve = (v_pve / s_vec)[vec_cat]
    s0 = 1 - s_pve + float((zz * v_pve / s_vec).sum())
    qvar = np.zeros((n_vc, n_vc))
    for i in range(n_vc):
        s1 = s0 - zwz[i] * (1 - s_pve) / s_vec[i]
        WXtXWz = XtXWz[:, i] * w_pve
        s1 -= (Xz_pve @ XWz[:, i]) / s_vec[i]
        for j in range(n_vc):
            s = s1 - zwz[j] * (1 - s_pve) / s_vec[j]
            s += (WXtXWz @ XtXWz[:, j]) / (s_vec[i] * s_vec[j])
            s += (XWz[:, i] @ XWz[:, j]) / (s_vec[i] * s_vec[j]) * (1 - s_pve)
            s -= (Xz_pve @ XWz[:, j]) / s_vec[j]
            qvar[i, j] = s
    d = float(ni_test - 1)
    qvar *= 2.0 / (d * d * d)
    Si = np.linalg.inv(S_mat)
    Var = np.zeros((n_vc, n_vc))
    for i in range(n_vc):
        for j in range(i, n_vc):
            Var[i, j] = Var[j, i] = Svar_mat[i, j] * (v_pve[i] * v_pve[j]) + qvar[i, j]
    Var = (Si @ Var) @ Si
    sigma2 = v_pve / s_vec
    enrich = v_pve / s_vec * s_snp / s_pve
    se_pve = np.sqrt(np.diag(Var))
    T = np.zeros((n_vc, n_vc))
    for i in range(n_vc):
        dd, d1 = v_pve[i] / s_pve, s_vec[i]
        for j in range(n_vc):
            T[i, j] = ((1 - dd) if i == j else (-1 * dd)) / d1 * s_snp / s_pve
    se_enrich = np.sqrt(np.diag((T @ Var) @ T.T))
    return dict(pve=v_pve.copy(), se_pve=se_pve, pve_total=s_pve, se_pve_total=float(np.sqrt(Var.sum())), sigma2=sigma2,
                se_sigma2=se_pve / s_vec, enrich=enrich, se_enrich=se_enrich)


def Calcq(n_block, vec_cat, vec_ni, vec_weight, vec_z2, n_vc):
    """src/gemma_io.cpp:3716-3870 -> (Vq, q, s): q per category and its block-jackknife variance over n_block SNP blocks, with the
    reference's `!= 0` tests and its halving of the off-diagonals."""
    n_vc, n_block = int(n_vc), int(n_block)
    Vq, q, s = np.zeros((n_vc, n_vc)), np.zeros(n_vc), np.zeros(n_vc)
    vec_q, vec_s, n_snps = [0.0] * n_vc, [0.0] * n_vc, [0.0] * n_vc
    cats = [int(c) for c in vec_cat]
    nis = [int(v) for v in vec_ni]
    ws = [float(v) for v in vec_weight]
    z2s = [float(v) for v in vec_z2]
    for cat, n_total, w, z2 in zip(cats, nis, ws, z2s):
        vec_q[cat] += (z2 - 1.0) * w / float(n_total)
        vec_s[cat] += w
        n_snps[cat] += 1
    for i in range(n_vc):
        if vec_s[i] != 0:
            q[i] = vec_q[i] / vec_s[i]
        s[i] = vec_s[i]
    for l in range(n_vc):
        n_snp = int(np.floor(n_snps[l] / n_block))
        t = b = 0
        if n_snp == 0:
            continue
        mat_q = [[0.0] * n_vc for _ in range(n_block)]
        mat_s = [[0.0] * n_vc for _ in range(n_block)]
        for cat, n_total, w, z2 in zip(cats, nis, ws, z2s):
            mat_q[b][cat] += (z2 - 1.0) * w
            mat_s[b][cat] += w
            if cat == l:
                if b < n_block - 1:
                    if t < n_snp - 1:
                        t += 1
                    else:
                        b += 1
                        t = 0
                else:
                    t += 1
        for i in range(n_vc):
            m = n = 0.0
            for k in range(n_block):
                if mat_s[k][i] != 0 and vec_s[i] != mat_s[k][i]:
                    d = (vec_q[i] - mat_q[k][i]) / (vec_s[i] - mat_s[k][i])
                    mat_q[k][i] = d
                    m += d
                    n += 1
            if n != 0:
                m /= n
            for k in range(n_block):
                if mat_q[k][i] != 0:
                    mat_q[k][i] -= m
        for i in range(n_vc):
            d = n = 0.0
            for k in range(n_block):
                if mat_q[k][l] != 0 and mat_q[k][i] != 0:
                    d += mat_q[k][l] * mat_q[k][i]
                    n += 1
            if n != 0:
                d /= n
                d *= n - 1
            d += Vq[i, l]
            Vq[i, l] = d
            if i != l:
                Vq[l, i] = d
    for i in range(n_vc):
        for j in range(i + 1, n_vc):
            d = Vq[i, j]
            Vq[i, j] = d / 2
            Vq[j, i] = d / 2
    return Vq, q, s


def CalcVCss(Vq, S_mat, Svar_mat, q_vec, s_vec, df):
    """src/vc.cpp:1309-1500 -> dict(pve, se_pve, pve_total, se_pve_total, sigma2, se_sigma2, enrich, se_enrich): the n_vc x n_vc
    algebra of the estimates; s_vec = the per-category SNP counts CalcS returned, df = ni_study."""
    S_mat, Svar_mat, Vq = np.asarray(S_mat, dtype=np.float64), np.asarray(Svar_mat, dtype=np.float64), np.asarray(Vq, dtype=np.float64)
    q_vec, s_vec = np.asarray(q_vec, dtype=np.float64), np.asarray(s_vec, dtype=np.float64)
    n_vc = S_mat.shape[0]
    Si = np.linalg.inv(S_mat)
    pve = Si @ q_vec
    sigma2 = pve / s_vec
    qvar = Vq / (df * df)
    Var = np.zeros((n_vc, n_vc))
    for i in range(n_vc):
        for j in range(i, n_vc):
            Var[i, j] = Var[j, i] = Svar_mat[i, j] * pve[i] * pve[j] + qvar[i, j]
    Var = (Si @ Var) @ Si
    se_pve = np.sqrt(np.diag(Var))
    se_sigma2 = se_pve / s_vec
    pve_total, se_pve_total = float(pve.sum()), float(np.sqrt(Var.sum()))
    s_pve, s_snp = pve.sum(), s_vec.sum()
    enrich = sigma2 * (s_snp / s_pve)
    T = np.zeros((n_vc, n_vc))
    for i in range(n_vc):
        d, d1 = pve[i] / s_pve, s_vec[i]
        for j in range(n_vc):
            T[i, j] = ((1 - d) if i == j else (-1 * d)) / d1 * s_snp / s_pve
    se_enrich = np.sqrt(np.diag((T @ Var) @ T.T))
    return dict(pve=pve, se_pve=se_pve, pve_total=pve_total, se_pve_total=se_pve_total, sigma2=sigma2, se_sigma2=se_sigma2,
                enrich=enrich, se_enrich=se_enrich)
