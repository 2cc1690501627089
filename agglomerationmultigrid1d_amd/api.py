"""Host-side mirror of the reference's operator interface for the V-cycle hot path.

The reference is Julia (no FFI of its own; Julia is not available in the build image), so the
host side above the C ABI is Python and mirrors the reference names, argument meaning, return
shapes and error behaviour:

    reference (Julia)                                   here
    --------------------------------------------------  -------------------------------------
    apply_smoother(S, B; alpha)    src/smoother.jl:6-81   apply_smoother(S, B, alpha=1.0)
    dg_smoother(mesh, A, :blockJac|:jac)  :142-168        dg_smoother(mesh, A, 'blockJac'|'jac')
    cg_smoother(mesh, A, :jac|:addSchwarz|:hybridSchwarz) cg_smoother(mesh, A, ...)
                                   :88-139
    struct MeshHierarchy           src/mesh_heirarchy.jl:17-28   class MeshHierarchy
    multigrid_v_cycle(H,x0,b;nPre,nPost,alpha) src/solvers.jl:19-50  multigrid_v_cycle(...)
    ldiv!(H,b) / ldiv!(y,H,b)      src/solvers.jl:63-92   ldiv(H, b) / ldiv(y, H, b)
    multigrid(H,x0,b,maxiter,tol)  src/solvers.jl:116-139 multigrid(...)
    iterative_smoother_solve(A,S,x0,b;maxiter,tol,alpha)  iterative_smoother_solve(...)
                                   src/solvers.jl:189-213

Julia Symbols become strings.  Every compute step goes through libaggmg_hip.so (include/
aggmg_hip.h); nothing here computes the hot path on the CPU.  Mesh arguments only need the
fields the reference reads on this path: `mElements[i].mNodesInd` (1-based) and `mP`, or a
ready `mBlockInds` array (see uniform.py for the O(n) descriptors used at scale).
"""
import ctypes

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import _lib
from ._lib import (ArgumentError, DimensionMismatch, check)

_PD = ctypes.POINTER(ctypes.c_double)
_PI64 = ctypes.POINTER(ctypes.c_int64)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _pd(a):
    return a.ctypes.data_as(_PD)


def device_memory():
    """(live allocations, live bytes) of device memory the library holds in this process (C ABI
    aggmg_debug_device_memory): what its handles and contexts own, not DeviceVector / DeviceMatrix storage.  Test aid."""
    n, b = ctypes.c_int64(), ctypes.c_int64()
    check(_lib.load().aggmg_debug_device_memory(ctypes.byref(n), ctypes.byref(b)), None)
    return n.value, b.value


# --------------------------------------------------------------------------------------------
# context
# --------------------------------------------------------------------------------------------
class Context:
    """One HIP device + stream (aggmg_create).  Not thread-safe, like the reference."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        check(self.lib.aggmg_create(int(device), ctypes.byref(h)), None)
        self.handle = h
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.aggmg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, status):
        check(status, self.handle)

    def synchronize(self):
        self.check(self.lib.aggmg_synchronize(self.handle))

    def set_option(self, option, value):
        """context options of the C ABI (aggmg_set_option), e.g. _lib.OPT_SYMMETRIC_PACKING"""
        self.check(self.lib.aggmg_set_option(self.handle, int(option), int(value)))
        self.__dict__.setdefault("_options", {})[int(option)] = int(value)

    def element_thread_launches(self):
        """launches of the element-thread kernel on this context so far (C ABI aggmg_element_thread_launches,
        AGGMG_OPT_ELEMENT_THREADS)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_element_thread_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def pair_element_thread_launches(self):
        """launches of the element-thread two-level kernels on this context so far (C ABI
        aggmg_pair_element_thread_launches, AGGMG_OPT_PAIR_ELEMENT_THREADS)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_pair_element_thread_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def replay_launches(self):
        """cycles of vcycle_dev that replayed their pre-smoothing on this context so far (C ABI aggmg_replay_launches,
        AGGMG_OPT_REPLAY_PRESMOOTH)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_replay_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def element_record_lds_launches(self):
        """launches of the element-thread kernels with the class records in LDS on this context so far (C ABI
        aggmg_element_record_lds_launches, AGGMG_OPT_ELEMENT_RECORDS_LDS)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_element_record_lds_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def element_record_lds_cap(self):
        """(cap on classes in force, largest cap the option takes) of AGGMG_OPT_ELEMENT_RECORDS_LDS (C ABI
        aggmg_element_record_lds_cap)"""
        c, m = ctypes.c_int(0), ctypes.c_int(0)
        self.check(self.lib.aggmg_element_record_lds_cap(self.handle, ctypes.byref(c), ctypes.byref(m)))
        return int(c.value), int(m.value)

    def coarse_dictionary_launches(self):
        """stage launches of the coarsest solve that read their factors from LDS on this context so far (C ABI
        aggmg_coarse_dictionary_launches, AGGMG_OPT_COARSE_DICTIONARY)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_coarse_dictionary_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def coarse_dictionary_cap(self):
        """(cap on classes in force, largest cap the option takes) of AGGMG_OPT_COARSE_DICTIONARY (C ABI
        aggmg_coarse_dictionary_cap)"""
        c, m = ctypes.c_int(0), ctypes.c_int(0)
        self.check(self.lib.aggmg_coarse_dictionary_cap(self.handle, ctypes.byref(c), ctypes.byref(m)))
        return int(c.value), int(m.value)

    def patch_multi_launches(self):
        """launches of the K-column multiplicative patch sweep kernel on this context so far (C ABI
        aggmg_patch_multi_launches; ElementPatchGaussSeidel.sweeps_multi_dev, AGGMG_OPT_PATCH_MULTI)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_patch_multi_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def patch_schwarz_multi_launches(self):
        """launches of the K-column hybrid / additive patch sweep kernel on this context so far (C ABI
        aggmg_patch_schwarz_multi_launches; ElementPatchSchwarz.sweeps_multi_dev and the hybrid patch levels of the
        K-column cycle, AGGMG_OPT_PATCH_SCHWARZ_MULTI); patch_multi_launches does not count them"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_patch_schwarz_multi_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def multi_element_thread_launches(self):
        """launches of the K-column element-thread kernel on this context so far (C ABI
        aggmg_multi_element_thread_launches; the dictionary levels of the K-column cycle under
        AGGMG_OPT_MULTI_ELEMENT_THREADS); element_thread_launches and element_record_lds_launches do not count them"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_multi_element_thread_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def chain_multi_launches(self):
        """launches of the K-column chain kernel on this context so far (C ABI aggmg_chain_multi_launches; the chain levels
        of the K-column cycle under AGGMG_OPT_CHAIN_MULTI)"""
        n = ctypes.c_int64(0)
        self.check(self.lib.aggmg_chain_multi_launches(self.handle, ctypes.byref(n)))
        return int(n.value)

    def option(self, option, default):
        """the value last given to set_option (the C ABI has no getter), `default` when it never was set"""
        return self.__dict__.get("_options", {}).get(int(option), default)

    def set_stream(self, hip_stream):
        """Launch on a caller-provided hipStream_t (integer / pointer), e.g.
        torch.cuda.current_stream().cuda_stream; 0 / None is the device's default stream."""
        self.check(self.lib.aggmg_set_stream(self.handle, ctypes.c_void_p(hip_stream or None)))

    def reset_stream(self):
        """back to the context's own non-blocking stream"""
        self.check(self.lib.aggmg_reset_stream(self.handle))

    # raw device vectors (harness plumbing; torch tensors' data_ptr() work equally well)
    def alloc(self, n):
        return DeviceVector(self, n)

    def to_device(self, x):
        x = _f64(x)
        v = DeviceVector(self, x.size)
        v.upload(x)
        return v

    def pin(self, x):
        """page-lock the memory of a NumPy array for good (C ABI aggmg_host_register): host-pointer calls that pass it
        -- multigrid_v_cycle(H, x0, b, out=), ldiv -- then move it by one DMA transfer instead of staging it.  The
        array must outlive the registration: unpin(x) (or freeing the context) ends it."""
        x = np.asarray(x)
        if x.dtype != np.float64 or not x.flags["C_CONTIGUOUS"]:
            raise ArgumentError("Context.pin: a C-contiguous float64 array")
        self.check(self.lib.aggmg_host_register(self.handle, ctypes.c_void_p(x.ctypes.data), x.nbytes))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[x.ctypes.data] = x      # (keeps the pages alive while they are registered)
        return x

    def unpin(self, x):
        self.check(self.lib.aggmg_host_unregister(self.handle, ctypes.c_void_p(x.ctypes.data)))
        getattr(self, "_pinned", {}).pop(x.ctypes.data, None)

    def pinned_empty(self, n):
        """float64 NumPy array of n entries in page-locked memory owned by the context (C ABI aggmg_host_alloc); freed
        with the context"""
        p = ctypes.c_void_p()
        self.check(self.lib.aggmg_host_alloc(self.handle, int(n) * 8, ctypes.byref(p)))
        buf = (ctypes.c_double * int(n)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.float64, count=int(n))

    def dot_cols(self, X, Y, n=None, ncols=None, ld=None):
        """X[:, j] . Y[:, j] for every column in one pass (C ABI aggmg_dot_cols_dev; EXTENSION): X, Y DeviceMatrix (or
        column-major device buffers with n, ncols, ld given); entry j is bit for bit dot() of column j.  -> array of K"""
        n, ncols, ld = _cols_shape("dot_cols", X, n, ncols, ld)
        if isinstance(Y, DeviceMatrix) and Y.shape != (n, ncols):
            raise DimensionMismatch("dot_cols: X and Y differ in shape")
        out = np.zeros(max(1, int(ncols)))
        self.check(self.lib.aggmg_dot_cols_dev(self.handle, _ptr(X), _ptr(Y), int(n), int(ncols), int(ld), _pd(out)))
        return out

    def norm2_cols(self, X, n=None, ncols=None, ld=None):
        """||X[:, j]||_2 for every column in one pass (C ABI aggmg_norm2_cols_dev; EXTENSION); entry j is bit for bit
        norm2() of column j.  -> array of K"""
        n, ncols, ld = _cols_shape("norm2_cols", X, n, ncols, ld)
        out = np.zeros(max(1, int(ncols)))
        self.check(self.lib.aggmg_norm2_cols_dev(self.handle, _ptr(X), int(n), int(ncols), int(ld), _pd(out)))
        return out

    def multi_dot(self, V, w, n=None, nvec=None, ld=None):
        """V[:, i] . w for every column of V with one pass over w per group of 8 columns (C ABI aggmg_multi_dot_dev;
        EXTENSION: the orthogonalisation of fgmres): V DeviceMatrix of at most 65 columns (or a column-major device
        buffer with n, nvec, ld given), w DeviceVector; entry i is bit for bit dot() of column i and w.
        -> array of nvec"""
        n, nvec, ld = _cols_shape("multi_dot", V, n, nvec, ld)
        if isinstance(w, DeviceVector) and w.n < n:
            raise DimensionMismatch("multi_dot: w is shorter than the columns of V")
        out = np.zeros(max(1, int(nvec)))
        self.check(self.lib.aggmg_multi_dot_dev(self.handle, _ptr(V), int(n), int(nvec), int(ld), _ptr(w), _pd(out)))
        return out

    def multi_axpy_norm(self, V, coef, w, n=None, nvec=None, ld=None, norm=True):
        """w += V @ coef in place, one fused multiply-add per column in ascending order, with one pass over w per group
        of 8 columns (C ABI aggmg_multi_axpy_norm_dev; EXTENSION: the orthogonalisation of fgmres).  -> ||w||_2 of the
        stored vector, summed by the pass that stores it (bit for bit norm2(w) afterwards); None with norm=False"""
        n, nvec, ld = _cols_shape("multi_axpy_norm", V, n, nvec, ld)
        if isinstance(w, DeviceVector) and w.n < n:
            raise DimensionMismatch("multi_axpy_norm: w is shorter than the columns of V")
        c = _f64(coef).ravel()
        if c.size != nvec:
            raise DimensionMismatch("multi_axpy_norm: one coefficient per column of V")
        out = ctypes.c_double(0.0)
        self.check(self.lib.aggmg_multi_axpy_norm_dev(self.handle, _ptr(V), int(n), int(nvec), int(ld), _pd(c), _ptr(w),
                                                      ctypes.byref(out) if norm else None))
        return out.value if norm else None

    def multi_dot_cols(self, V, W, n, nvec, ncols, bstride=None, cstride=None, ldw=None):
        """V_i[:, c] . W[:, c] for nvec basis vectors of each of ncols independent bases, all in one launch sequence (C
        ABI aggmg_multi_dot_cols_dev; EXTENSION: the orthogonalisation of fgmres_multi).  V a device buffer with basis
        vector i of column c at offset i * bstride + c * cstride (defaults: cstride = n, bstride = n * ncols), W column
        c at offset c * ldw (default n).  -> array (ncols, nvec); entry (c, i) is bit for bit multi_dot's entry i on
        column c alone"""
        n, nvec, ncols = int(n), int(nvec), int(ncols)
        cstride = n if cstride is None else int(cstride)
        bstride = cstride * ncols if bstride is None else int(bstride)
        ldw = n if ldw is None else int(ldw)
        out = np.zeros((max(1, ncols), max(1, nvec)))
        self.check(self.lib.aggmg_multi_dot_cols_dev(self.handle, _ptr(V), n, nvec, ncols, bstride, cstride, _ptr(W), ldw,
                                                     _pd(out)))
        return out[:max(0, ncols), :max(0, nvec)]

    def multi_axpy_norm_cols(self, V, coef, W, n, nvec, ncols, bstride=None, cstride=None, ldw=None, norm=True):
        """W[:, c] += V_c @ coef[c] in place for ncols independent bases, one fused multiply-add per basis vector in
        ascending order (C ABI aggmg_multi_axpy_norm_cols_dev; EXTENSION: the orthogonalisation of fgmres_multi); the
        layout is multi_dot_cols', coef an (ncols, nvec) array.  -> array of the ncols norms of the stored columns, each
        summed by the pass that stores it (bit for bit multi_axpy_norm on column c alone); None with norm=False"""
        n, nvec, ncols = int(n), int(nvec), int(ncols)
        cstride = n if cstride is None else int(cstride)
        bstride = cstride * ncols if bstride is None else int(bstride)
        ldw = n if ldw is None else int(ldw)
        c = np.ascontiguousarray(_f64(coef))
        if nvec >= 1 and ncols >= 1 and c.shape != (ncols, nvec):
            raise DimensionMismatch("multi_axpy_norm_cols: coef must have shape (ncols, nvec)")
        out = np.zeros(max(1, ncols))
        self.check(self.lib.aggmg_multi_axpy_norm_cols_dev(self.handle, _ptr(V), n, nvec, ncols, bstride, cstride, _pd(c),
                                                           _ptr(W), ldw, _pd(out) if norm else None))
        return out[:max(0, ncols)] if norm else None

    def profile_enable(self, on=True):
        """True / 1: HIP events around every launch; 2: only the fine-level fused-down launch;
        False / 0: off"""
        self.check(self.lib.aggmg_profile_enable(self.handle, int(on)))

    def profile_collect(self):
        """-> {(kind_name, level): (total_ms, count)} for every tag seen since the last call."""
        ms = np.zeros(_lib.PROFILE_NTAGS)
        cnt = np.zeros(_lib.PROFILE_NTAGS, dtype=np.int64)
        self.check(self.lib.aggmg_profile_collect(self.handle, _pd(ms), cnt.ctypes.data_as(_PI64)))
        out = {}
        for tag in np.nonzero(cnt)[0]:
            out[(_lib.KIND_NAMES[tag // 16], int(tag % 16))] = (float(ms[tag]), int(cnt[tag]))
        return out


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class _DevPtr(ctypes.c_void_p):
    """Device address handed out by DeviceVector.ptr.  It keeps its vector referenced for as long as the pointer object
    itself lives -- the argument tuple of a ctypes call included -- so `ctx.to_device(x).ptr` passed straight into a
    `*_dev` entry point cannot be finalised (aggmg_dev_free) before the call has enqueued its launches; the free that
    follows synchronises the context's stream first (aggmg_dev_free), i.e. it waits for them.  (r03: such a temporary was
    freed between `.ptr` and the launch -- a dangling device pointer, a memory access fault on the GPU.)"""
    _owner = None


class DeviceVector:
    """fp64 vector in HBM owned by a Context.  `.ptr` is the device address (a c_void_p that keeps the vector alive);
    after free() it raises instead of yielding a stale address."""

    def __init__(self, ctx, n):
        self.ctx = ctx
        self.n = int(n)
        self._p = None
        p = ctypes.c_void_p()
        ctx.check(ctx.lib.aggmg_dev_alloc(ctx.handle, self.n * 8, ctypes.byref(p)))
        self._p = p

    @property
    def ptr(self):
        if self._p is None:
            raise ArgumentError("DeviceVector: used after free() -- its device memory has been released")
        q = _DevPtr(self._p.value)
        q._owner = self
        return q

    def upload(self, x):
        x = _f64(x)
        if x.size != self.n:
            raise DimensionMismatch("DeviceVector.upload: size mismatch")
        self.ctx.check(self.ctx.lib.aggmg_memcpy_h2d(self.ctx.handle, self.ptr, x.ctypes.data, x.size * 8))

    def download(self):
        out = np.empty(self.n)
        self.ctx.check(self.ctx.lib.aggmg_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, self.n * 8))
        return out

    def free(self):
        """release the device memory (waits for the launches already enqueued on the context's stream)"""
        p, self._p = self._p, None
        if p is not None and self.ctx.handle:
            self.ctx.lib.aggmg_dev_free(self.ctx.handle, p)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceMatrix:
    """fp64 N x K matrix in HBM owned by a Context, column-major (column j at `.ptr + 8 j N`), for the K-column cycle
    (MeshHierarchy.vcycle_multi_dev; EXTENSION).  Same lifetime rules as DeviceVector: `.ptr` keeps the matrix alive,
    after free() it raises."""

    def __init__(self, ctx, n, k):
        self.ctx = ctx
        self.n = int(n)
        self.k = int(k)
        if self.n < 0 or self.k < 1:
            raise ArgumentError("DeviceMatrix: needs n >= 0 rows and k >= 1 columns")
        self._p = None
        p = ctypes.c_void_p()
        ctx.check(ctx.lib.aggmg_dev_alloc(ctx.handle, self.n * self.k * 8, ctypes.byref(p)))
        self._p = p

    @property
    def shape(self):
        return (self.n, self.k)

    @property
    def ptr(self):
        if self._p is None:
            raise ArgumentError("DeviceMatrix: used after free() -- its device memory has been released")
        q = _DevPtr(self._p.value)
        q._owner = self
        return q

    def upload(self, X):
        X = np.asarray(X, dtype=np.float64)
        if X.shape != (self.n, self.k):
            raise DimensionMismatch(f"DeviceMatrix.upload: shape {X.shape}, expected {(self.n, self.k)}")
        F = np.asfortranarray(X)
        self.ctx.check(self.ctx.lib.aggmg_memcpy_h2d(self.ctx.handle, self.ptr, F.ctypes.data, F.size * 8))

    def download(self):
        out = np.empty((self.n, self.k), order="F")
        self.ctx.check(self.ctx.lib.aggmg_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, out.size * 8))
        return out

    def free(self):
        """release the device memory (waits for the launches already enqueued on the context's stream)"""
        p, self._p = self._p, None
        if p is not None and self.ctx.handle:
            self.ctx.lib.aggmg_dev_free(self.ctx.handle, p)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _cols_shape(who, X, n, ncols, ld):
    """(n, ncols, ld) of a column-major device matrix: a DeviceMatrix's own, or what the caller gives for a raw buffer"""
    if isinstance(X, DeviceMatrix):
        n = X.n if n is None else n
        ncols = X.k if ncols is None else ncols
    if n is None or ncols is None:
        raise ArgumentError(f"{who}: n and ncols are needed for raw device pointers")
    return int(n), int(ncols), int(n if ld is None else ld)


def _ptr(v):
    """device pointer of a DeviceVector / DeviceMatrix / torch tensor / int"""
    if v is None:
        return ctypes.c_void_p(None)
    if isinstance(v, (DeviceVector, DeviceMatrix)):
        return v.ptr
    if hasattr(v, "data_ptr"):
        return ctypes.c_void_p(v.data_ptr())
    return ctypes.c_void_p(int(v))


# --------------------------------------------------------------------------------------------
# operators
# --------------------------------------------------------------------------------------------
class DeviceOperator:
    """Device mirror of one SparseMatrixCSC{Float64,Int64} (H.mStiffness[k] / H.mInterpolation[k],
    src/mesh_heirarchy.jl:20,26).  `A` is a SciPy sparse matrix or the Julia triple
    (m, n, colptr, rowval, nzval) with 1-based Int64 indices (a sixth entry 0 marks 0-based index arrays)."""

    def __init__(self, A, kind=_lib.OP_STIFFNESS, ctx=None):
        self.ctx = ctx or default_context()
        if isinstance(A, tuple):
            # (m, n, colptr, rowval, nzval[, one_based]): the arrays of a SparseMatrixCSC as they lie in memory
            m, n, colptr, rowval, nzval = A[:5]
            one_based = int(A[5]) if len(A) > 5 else 1
        else:
            if isinstance(A, np.ndarray) and A.ndim == 2:
                # a dense Matrix{Float64} in mInterpolation::Vector{AbstractMatrix{Float64}} (src/mesh_heirarchy.jl:26;
                # dg_cg_interpolation(..., 0) returns one): its non-zero entries as a CSC operator -- `L * v` and
                # `L' * v` add the same products in the same order
                A = sp.csc_matrix(A)
            elif not sp.issparse(A):
                raise ArgumentError("DeviceOperator: a SparseMatrixCSC (SciPy sparse matrix), the (m, n, colptr, rowval, "
                                    "nzval) arrays of one, or a dense 2-D array")
            A = sp.csc_matrix(A)
            A.sort_indices()
            m, n = A.shape
            colptr, rowval, nzval = A.indptr, A.indices, A.data
            one_based = 0
        colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        rowval = np.ascontiguousarray(rowval, dtype=np.int64)
        nzval = _f64(nzval)
        # the C ABI takes pointers: it reads colptr[n] and then colptr[n] - base entries of rowval and nzval whatever
        # the arrays hold, so what only the array lengths can tell is checked here
        if int(m) < 0 or int(n) < 0:
            raise ArgumentError("DeviceOperator: negative dimension")
        if colptr.ndim != 1 or colptr.size != int(n) + 1:
            raise ArgumentError(f"DeviceOperator: colptr must hold n + 1 = {int(n) + 1} entries, not {colptr.size}")
        nnz = int(colptr[int(n)]) - (1 if one_based else 0)
        if nnz < 0 or nnz > min(rowval.size, nzval.size):
            raise ArgumentError(f"DeviceOperator: colptr ends at {nnz} entries, rowval and nzval hold "
                                f"{rowval.size} and {nzval.size}")
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.aggmg_csc_upload(
            self.ctx.handle, int(m), int(n), colptr.ctypes.data_as(_PI64), rowval.ctypes.data_as(_PI64),
            _pd(nzval), one_based, int(kind), ctypes.byref(h)))
        self.handle = h
        self.shape = (int(m), int(n))
        self.nnz = nnz        # (a SparseMatrixCSC may carry rowval / nzval longer than its colptr uses)
        self.kind = kind

    @classmethod
    def _from_handle(cls, ctx, handle, kind):
        """wrap an operator the library produced (aggmg_sp_matmul, aggmg_bd_sp_apply, ...)"""
        self = cls.__new__(cls)
        self.ctx, self.handle, self.kind = ctx, handle, kind
        m, n, nnz = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        ctx.check(ctx.lib.aggmg_op_shape(ctx.handle, handle, ctypes.byref(m), ctypes.byref(n), ctypes.byref(nnz)))
        self.shape, self.nnz = (m.value, n.value), nnz.value
        return self

    def to_scipy(self):
        """the operator as a SciPy CSC matrix (C ABI aggmg_op_download_csc): stored entries, zeros included"""
        cp = np.empty(self.shape[1] + 1, dtype=np.int32)
        rv = np.empty(self.nnz, dtype=np.int32)
        nz = np.empty(self.nnz)
        self.ctx.check(self.ctx.lib.aggmg_op_download_csc(
            self.ctx.handle, self.handle, cp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            rv.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _pd(nz)))
        return sp.csc_matrix((nz, rv, cp), shape=self.shape)

    def _binary(self, fn, other, kind):
        other = _as_op(other, kind, self.ctx)
        h = ctypes.c_void_p()
        self.ctx.check(fn(self.ctx.handle, self.handle, other.handle, int(kind), ctypes.byref(h)))
        return DeviceOperator._from_handle(self.ctx, h, kind)

    def matmul(self, B, kind=_lib.OP_STIFFNESS):
        """`A * B` for two sparse matrices on the device (C ABI aggmg_sp_matmul): the products of
        `L'*X*L` and `D*(M_LU\\G)`, src/mesh_heirarchy.jl:71-72,79-84"""
        return self._binary(self.ctx.lib.aggmg_sp_matmul, B, kind)

    def sub(self, B, kind=_lib.OP_STIFFNESS):
        """`A - B`, numerically-zero results dropped as SparseArrays does (C ABI aggmg_sp_sub)"""
        return self._binary(self.ctx.lib.aggmg_sp_sub, B, kind)

    def transpose(self, kind=_lib.OP_STIFFNESS):
        """the adjoint as an operator of its own (C ABI aggmg_op_transpose)"""
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.aggmg_op_transpose(self.ctx.handle, self.handle, int(kind), ctypes.byref(h)))
        return DeviceOperator._from_handle(self.ctx, h, kind)

    def download(self, transposed=False):
        """Device index maps and values: (rowptr, colind, vals), 0-based int32 CSR of the matrix
        (or of its transpose)."""
        nrows = self.shape[1] if transposed else self.shape[0]
        rp = np.empty(nrows + 1, dtype=np.int32)
        ci = np.empty(self.nnz, dtype=np.int32)
        v = np.empty(self.nnz)
        self.ctx.check(self.ctx.lib.aggmg_op_download(
            self.ctx.handle, self.handle, 1 if transposed else 0,
            rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            ci.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _pd(v)))
        return rp, ci, v

    def release_host(self):
        self.ctx.check(self.ctx.lib.aggmg_op_release_host(self.ctx.handle, self.handle))

    def residual_multi_dev(self, X, B, R, ncols=None, ld=None):
        """R = B - A X on K columns (C ABI aggmg_residual_multi_dev; EXTENSION): X, B (None: R = -A X), R DeviceMatrix /
        column-major device buffers with leading dimension ld (default N); column j of R is bit for bit the single-vector
        residual of column j.  Asynchronous on the context stream."""
        N = self.shape[0]
        if ncols is None:
            ncols = X.k if isinstance(X, DeviceMatrix) else None
        if ncols is None:
            raise ArgumentError("residual_multi_dev: ncols is needed for raw device pointers")
        for M_ in (X, B, R):   # (ncols < 1, ld < N: the C ABI's ArgumentError)
            if isinstance(M_, DeviceMatrix) and int(ncols) >= 1 and (M_.n != N or M_.k < int(ncols)):
                raise DimensionMismatch("residual_multi_dev: matrix shape does not match (N, ncols)")
        c = self.ctx
        c.check(c.lib.aggmg_residual_multi_dev(c.handle, self.handle, _ptr(X), _ptr(B), int(ncols), int(N if ld is None else ld),
                                               _ptr(R)))

    def residual_multi_launch_bytes(self, K, has_b=True):
        """(read, write) compulsory HBM bytes of one K-column residual launch (C ABI aggmg_residual_multi_launch_bytes):
        the operator's entry arrays once, the vectors once per column"""
        r, w = ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.check(self.ctx.lib.aggmg_residual_multi_launch_bytes(self.ctx.handle, self.handle, int(K), int(bool(has_b)),
                                                                      ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def free(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.lib.aggmg_op_free(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_op(A, kind=_lib.OP_STIFFNESS, ctx=None):
    return A if isinstance(A, DeviceOperator) else DeviceOperator(A, kind, ctx)


# --------------------------------------------------------------------------------------------
# smoothers (src/smoother.jl)
# --------------------------------------------------------------------------------------------
class AbstractSmoother:
    """abstract type AbstractSmoother (src/AgglomerationMultigrid1D.jl:16)"""
    handle = None

    def free(self):
        if getattr(self, "handle", None) and self.A.ctx.handle:
            self.A.ctx.lib.aggmg_smoother_free(self.A.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def structured(self):
        out = ctypes.c_int(0)
        c = self.A.ctx
        c.check(c.lib.aggmg_smoother_is_structured(c.handle, self.handle, ctypes.byref(out)))
        return bool(out.value)


class JacobiSmoother(AbstractSmoother):
    """JacobiSmoother{mJac::Diagonal} src/smoother.jl:52-58.

    mElementNodes: optional (p+1) x n matrix of the CG mesh's element node lists (1-based, column k
    = cgMesh.mElements[k].mNodesInd, src/cg_mesh.jl:35-45) -- what cg_smoother(cgMesh, A, :jac) has at
    hand.  Same smoother; with the lists the level also gets the element-contiguous chain form and
    runs the fused point-Jacobi kernel (C ABI aggmg_jacobi_setup_elements).
    Without lists the library looks at the operator itself (AGGMG_OPT_DETECT_CHAIN): a CG operator in the reference's
    vertices-first numbering is recognised from its pattern and takes the same chain kernels; detect=False keeps an
    operator without lists on the generic CSR kernels whatever its pattern."""

    def __init__(self, A, ctx=None, mElementNodes=None, detect=True):
        self.A = _as_op(A, ctx=ctx)
        h = ctypes.c_void_p()
        c = self.A.ctx
        if mElementNodes is None:
            was = c.option(_lib.OPT_DETECT_CHAIN, 1)
            if not detect and was:
                c.set_option(_lib.OPT_DETECT_CHAIN, 0)
            try:
                c.check(c.lib.aggmg_jacobi_setup(c.handle, self.A.handle, ctypes.byref(h)))
            finally:
                if not detect and was:
                    c.set_option(_lib.OPT_DETECT_CHAIN, was)
        else:
            inds = np.asarray(mElementNodes, dtype=np.int64)
            if inds.ndim != 2:
                raise ArgumentError("mElementNodes must be a ((p+1) x n) matrix")
            m1, n = inds.shape
            flat = np.ascontiguousarray(inds.T)     # column-major (p+1) x n == C-order n x (p+1)
            c.check(c.lib.aggmg_jacobi_setup_elements(c.handle, self.A.handle, m1, n, flat.ctypes.data_as(_PI64), 1,
                                                      ctypes.byref(h)))
        self.handle = h


class _BlockSmoother(AbstractSmoother):
    _kind = 0

    def __init__(self, A, mBlockInds, ctx=None):
        """mBlockInds: Matrix{Int64}(m x nb), 1-based, column i = index list of block i
        (src/smoother.jl:13,76)."""
        self.A = _as_op(A, ctx=ctx)
        inds = np.asarray(mBlockInds, dtype=np.int64)
        if inds.ndim != 2:
            raise ArgumentError("mBlockInds must be an (m x nb) matrix")
        self.mBlockInds = inds
        m, nb = inds.shape
        flat = np.ascontiguousarray(inds.T)  # column-major m x nb == C-order nb x m
        h = ctypes.c_void_p()
        c = self.A.ctx
        c.check(c.lib.aggmg_blockjacobi_setup(c.handle, self.A.handle, m, nb,
                                              flat.ctypes.data_as(_PI64), 1, self._kind,
                                              ctypes.byref(h)))
        self.handle = h

    def inverse_blocks(self):
        """the explicit inverses of the pivoted block LUs, (nb, m, m): what the device factorisation (K6)
        produced from A[inds, inds] (C ABI aggmg_smoother_download_blocks)"""
        m, nb = self.mBlockInds.shape
        return _download_blocks(self.A.ctx, self.handle, nb, m)


def _download_blocks(ctx, handle, nb, m):
    out = np.empty((nb, m, m))
    ctx.check(ctx.lib.aggmg_smoother_download_blocks(ctx.handle, handle, _pd(out)))
    return out


class BlockJacobi(_BlockSmoother):
    """BlockJacobi{mBlocks::Vector{LU}, mBlockInds} src/smoother.jl:64-81.  Blocks are
    re-extracted from A on set-up (identical mathematics to src/smoother.jl:159-162)."""


class AdditiveSchwarzSmoother(_BlockSmoother):
    """src/smoother.jl:1-18 (same apply loop as BlockJacobi, overlapping blocks)"""


class BlockGaussSeidel(_BlockSmoother):
    """EXTENSION: red-black block Gauss-Seidel on a block-tridiagonal operator (C ABI kind 2 of
    aggmg_blockjacobi_setup).  The reference has no Gauss-Seidel smoother;
    BASELINE.json names one, so it is offered and checked against the oracle's restatement
    (BlockGaussSeidelRB), not against the reference.  Also on the overlapping element blocks of a CG mesh
    (cg_smoother(mesh, A, 'blockGS'): elements of one colour share no node).  One sweep: even elements, then odd ones, each
    with the newest values; V-cycles post-smooth in the reverse order.  UnsupportedError unless the
    blocks are contiguous and the operator couples an element to its direct neighbours only."""
    _kind = 2


class HybridSchwarzSmoother(_BlockSmoother):
    """src/smoother.jl:24-46"""
    _kind = 1


def element_patch_lists(m, ne, width=2):
    """index lists (1-based, (w m) x nb, column e = patch {e, .., e + w - 1}, w = min(width, ne)) of the element
    patches ElementPatchSchwarz smooths with: what HybridSchwarzSmoother(A, lists) takes for the same smoother"""
    w = min(int(width), int(ne))
    nb = int(ne) - w + 1
    return np.arange(nb, dtype=np.int64)[None, :] * int(m) + np.arange(1, w * int(m) + 1, dtype=np.int64)[:, None]


class ElementPatchSchwarz(AbstractSmoother):
    """EXTENSION: Schwarz smoother of a DG level on overlapping patches of `width` consecutive elements (C ABI
    aggmg_patch_schwarz_setup) -- the arithmetic of HybridSchwarzSmoother (hybrid=True: the summed patch corrections
    divided by the number of patches covering the element, src/smoother.jl:24-46) or AdditiveSchwarzSmoother
    (hybrid=False) on element_patch_lists(m, ne, width).  width = 2 on an operator that is block tridiagonal in the
    blocking of ne elements of m rows runs the fused, LDS-tiled sweep kernel (`.fused`); everything else the generic
    kernels on the lists, with the same results to round-off.
    The smoothed cycle is not a symmetric preconditioner: use fgmres, not pcg, around it -- or ElementPatchGaussSeidel,
    the multiplicative sweeps over the same patches, whose cycle is symmetric when nPre == nPost and the post weights
    are the pre weights reversed."""

    def __init__(self, A, m, ne, width=2, hybrid=True, ctx=None):
        self.A = _as_op(A, ctx=ctx)
        self.m, self.ne = int(m), int(ne)
        h = ctypes.c_void_p()
        c = self.A.ctx
        c.check(c.lib.aggmg_patch_schwarz_setup(c.handle, self.A.handle, self.m, self.ne, int(width), int(bool(hybrid)),
                                                ctypes.byref(h)))
        self.handle = h
        w, hy, fu = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        c.check(c.lib.aggmg_smoother_patch_info(c.handle, h, ctypes.byref(w), ctypes.byref(hy), ctypes.byref(fu)))
        self.width, self.hybrid, self.fused = w.value, bool(hy.value), bool(fu.value)
        # distinct operator records of the fused form's dictionary (AGGMG_OPT_OPERATOR_DICTIONARY; C ABI
        # aggmg_smoother_patch_dictionary): 0 = the sweeps read the full arrays
        nc = ctypes.c_int(0)
        c.check(c.lib.aggmg_smoother_patch_dictionary(c.handle, h, ctypes.byref(nc)))
        self.dictionary_classes = nc.value
        self.mBlockInds = element_patch_lists(self.m, self.ne, self.width)

    def inverse_blocks(self):
        """the explicit inverses of the patch blocks, (nb, w m, w m) (C ABI aggmg_smoother_download_blocks)"""
        bm, nb = self.mBlockInds.shape
        return _download_blocks(self.A.ctx, self.handle, nb, bm)

    def sweeps_multi_dev(self, U0, B, U, weights, ncols=None, ld=None):
        """len(weights) sweeps on K columns in one pass over the operator per column group (C ABI aggmg_smooth_multi_dev
        under AGGMG_OPT_PATCH_SCHWARZ_MULTI; EXTENSION): U0 (None: the zero iterate), B, U are DeviceMatrix / column-major
        device buffers with leading dimension ld (default N); sweep s is damped by weights[s].  The sweeps have no
        direction (the C entry point's `reverse` is ignored for this smoother).  Column j of U is bit for bit the
        single-column sweeps of column j.  UnsupportedError with the option off, for a smoother on the generic route
        (width 3 or 4, or not `.fused`) and for element blocks outside the kernel's coverage (compressed couplings with 2
        or 4 rows, dense ones with 2).  Asynchronous on the context stream."""
        N = self.m * self.ne
        if ncols is None:
            ncols = B.k if isinstance(B, DeviceMatrix) else None
        if ncols is None:
            raise ArgumentError("sweeps_multi_dev: ncols is needed for raw device pointers")
        if ld is None:
            ld = N
        w = np.ascontiguousarray(np.atleast_1d(weights), dtype=np.float64)
        c = self.A.ctx
        c.check(c.lib.aggmg_smooth_multi_dev(c.handle, self.A.handle, self.handle, _ptr(U0), _ptr(B), int(ncols), int(ld),
                                             w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(w.size), 0, _ptr(U)))


class ElementPatchGaussSeidel(AbstractSmoother):
    """EXTENSION: multiplicative two-colour smoother of a DG level on the patches {e, e + 1} of two consecutive elements
    (C ABI aggmg_patch_gs_setup): a forward sweep of weight w is, for the colours c = 0, 1,
    r = b - A u and u[P_e] += w inv(A[P_e, P_e]) r[P_e] for every patch e = c (mod 2); post-smoothing runs the colours
    in reverse order.  The same inverses, element blocks and dictionary records as ElementPatchSchwarz, in a fused
    sweep kernel of its own; there is no generic route (UnsupportedError where the operator is not block tridiagonal in
    the blocking of ne >= 2 elements of m rows, or m is not instantiated).
    The smoothed cycle is a symmetric preconditioner when nPre == nPost and the post weights are the pre weights
    reversed: pcg is valid around it."""

    def __init__(self, A, m, ne, ctx=None):
        self.A = _as_op(A, ctx=ctx)
        self.m, self.ne = int(m), int(ne)
        h = ctypes.c_void_p()
        c = self.A.ctx
        c.check(c.lib.aggmg_patch_gs_setup(c.handle, self.A.handle, self.m, self.ne, ctypes.byref(h)))
        self.handle = h
        kind, nc = ctypes.c_int(0), ctypes.c_int(0)
        c.check(c.lib.aggmg_smoother_patch_kind(c.handle, h, ctypes.byref(kind)))
        c.check(c.lib.aggmg_smoother_patch_dictionary(c.handle, h, ctypes.byref(nc)))
        self.width, self.fused, self.kind = 2, kind.value == 3, kind.value
        self.dictionary_classes = nc.value   # 0: the sweeps read the full arrays
        self.mBlockInds = element_patch_lists(self.m, self.ne, 2)

    def inverse_blocks(self):
        """the explicit inverses of the patch blocks, (ne - 1, 2 m, 2 m) (C ABI aggmg_smoother_download_blocks)"""
        bm, nb = self.mBlockInds.shape
        return _download_blocks(self.A.ctx, self.handle, nb, bm)

    def sweeps_multi_dev(self, U0, B, U, weights, reverse=False, ncols=None, ld=None):
        """len(weights) sweeps on K columns in one pass over the operator per column group (C ABI aggmg_smooth_multi_dev;
        EXTENSION): U0 (None: the zero iterate), B, U are DeviceMatrix / column-major device buffers with leading
        dimension ld (default N); sweep s is damped by weights[s]; reverse: the colour order of post-smoothing.  Column j
        of U is bit for bit the single-column sweeps of column j.  UnsupportedError for element blocks outside the
        kernel's coverage (compressed couplings with 2 or 4 rows, dense ones with 2).  Asynchronous on the context
        stream."""
        N = self.m * self.ne
        if ncols is None:
            ncols = B.k if isinstance(B, DeviceMatrix) else None
        if ncols is None:
            raise ArgumentError("sweeps_multi_dev: ncols is needed for raw device pointers")
        if ld is None:
            ld = N
        w = np.ascontiguousarray(np.atleast_1d(weights), dtype=np.float64)
        c = self.A.ctx
        c.check(c.lib.aggmg_smooth_multi_dev(c.handle, self.A.handle, self.handle, _ptr(U0), _ptr(B), int(ncols), int(ld),
                                             w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(w.size), 1 if reverse else 0,
                                             _ptr(U)))


class _BlockObject(AbstractSmoother):
    """device handle of a block-diagonal matrix or of its factorisation"""

    def __init__(self, ctx, handle, N):
        self._ctx, self.handle, self.N = ctx, handle, N

    def free(self):
        if getattr(self, "handle", None) and self._ctx.handle:
            self._ctx.lib.aggmg_smoother_free(self._ctx.handle, self.handle)
        self.handle = None

    def _apply_sparse(self, S, kind):
        """block object times a sparse matrix -> DeviceOperator (C ABI aggmg_bd_sp_apply)"""
        S = _as_op(S, kind, self._ctx)
        h = ctypes.c_void_p()
        c = self._ctx
        c.check(c.lib.aggmg_bd_sp_apply(c.handle, self.handle, S.handle, int(kind), ctypes.byref(h)))
        return DeviceOperator._from_handle(c, h, kind)

    def _apply(self, B):
        B = np.asarray(B, dtype=np.float64)
        if B.ndim not in (1, 2) or B.shape[0] != self.N:
            raise DimensionMismatch("BlockDiagonal: DimensionMismatch")
        ncols = 1 if B.ndim == 1 else B.shape[1]
        Bf = np.asfortranarray(B.reshape(self.N, ncols))
        Y = np.empty((self.N, ncols), order='F')
        c = self._ctx
        c.check(c.lib.aggmg_smoother_apply(c.handle, self.handle, Bf.ctypes.data_as(_PD), self.N, ncols, 1.0,
                                           Y.ctypes.data_as(_PD)))
        return Y[:, 0].copy() if B.ndim == 1 else np.ascontiguousarray(Y)


class BlockDiagonal:
    """struct BlockDiagonal{mBlocks, mBlockSize, mBlockInds} (src/block_diagonal.jl:11-15) with the
    BlockDiagonal(mBlocks) constructor (:27-41): equal-sized dense blocks, contiguous index lists.
    `A * x` / `A * B` for dense vectors and matrices run the batched block kernel (mul!, :166-176);
    `lu(A)` (:276) gives a BlockDiagonalLU."""

    def __init__(self, mBlocks, ctx=None):
        if len(mBlocks) == 0:
            raise ArgumentError("BlockDiagonal needs at least one block")
        if isinstance(mBlocks, np.ndarray) and mBlocks.ndim == 3:
            # the blocks as one (nb, m, m) array (what the vectorised builders produce): no per-block Python work
            if mBlocks.shape[1] != mBlocks.shape[2]:
                raise ArgumentError("All blocks must be of the same size.")
            m = mBlocks.shape[1]
            self.mBlocks = np.ascontiguousarray(mBlocks, dtype=np.float64)
        else:
            m = np.asarray(mBlocks[0]).shape[0]
            for blk in mBlocks:
                if np.asarray(blk).shape != (m, m):
                    raise ArgumentError("All blocks must be of the same size.")   # block_diagonal.jl:35-37
            self.mBlocks = [np.array(blk, dtype=np.float64) for blk in mBlocks]
        self.mBlockSize = m
        nb = len(mBlocks)
        self.mBlockInds = np.arange(nb, dtype=np.int64)[None, :] * m + np.arange(1, m + 1, dtype=np.int64)[:, None]
        self._ctx = ctx or default_context()
        self._dev = None

    @property
    def shape(self):
        n = len(self.mBlocks) * self.mBlockSize
        return (n, n)

    def _setup(self, factorize):
        c = self._ctx
        if isinstance(self.mBlocks, np.ndarray):
            flat = np.ascontiguousarray(np.transpose(self.mBlocks, (0, 2, 1)))
        else:
            flat = np.ascontiguousarray(np.stack([b.T for b in self.mBlocks]))   # column-major per block
        h = ctypes.c_void_p()
        c.check(c.lib.aggmg_blockdiag_setup(c.handle, self.mBlockSize, len(self.mBlocks), flat.ctypes.data_as(_PD),
                                            1 if factorize else 0, ctypes.byref(h)))
        return _BlockObject(c, h, self.shape[0])

    def __matmul__(self, B):
        """`A * x`, `A * B` (dense: mul!, :166-176) and `A * S` for a sparse S (SciPy sparse or DeviceOperator:
        bd_sp_matmul, :195-264 -> DeviceOperator)"""
        if self._dev is None:
            self._dev = self._setup(False)
        if sp.issparse(B) or isinstance(B, DeviceOperator):
            return self._dev._apply_sparse(B, _lib.OP_STIFFNESS)
        return self._dev._apply(B)

    mul = __matmul__

    def lu(self):
        return BlockDiagonalLU(self)

    def todense(self):
        """Matrix(A) (src/block_diagonal.jl:107-114)"""
        out = np.zeros(self.shape)
        m = self.mBlockSize
        for k, blk in enumerate(self.mBlocks):
            out[k * m:(k + 1) * m, k * m:(k + 1) * m] = blk
        return out


class BlockDiagonalLU:
    """struct BlockDiagonalLU (src/block_diagonal.jl:17-21, ctor :47-58): `A \\ x`, `A \\ B` for dense
    right-hand sides (ldiv!, :299-309).  A singular block raises SingularException."""

    def __init__(self, A):
        self.mBlockSize, self.mBlockInds = A.mBlockSize, A.mBlockInds
        self._dev = A._setup(True)

    @property
    def shape(self):
        return (self._dev.N, self._dev.N)

    def solve(self, B, kind=_lib.OP_STIFFNESS):
        """`A \\ x`, `A \\ B` (dense: ldiv!, :299-309) and `A \\ S` for a sparse S (bd_sp_solve, :314-383
        -> DeviceOperator).  Deviation from the reference's operation sequence: every block's pivoted LU is turned
        into an explicit inverse once and applied by multiplication (the reference runs getrs per block and column,
        src/block_diagonal.jl:305,374): equal to round-off for the well-conditioned mass blocks of the hierarchy
        constructors, checked against the oracle at 1e-12."""
        if sp.issparse(B) or isinstance(B, DeviceOperator):
            return self._dev._apply_sparse(B, kind)
        return self._dev._apply(B)

    ldiv = solve


def _mesh_block_inds(mesh):
    if hasattr(mesh, "mBlockInds"):
        return np.asarray(mesh.mBlockInds, dtype=np.int64)
    n = len(mesh.mElements)
    inds = np.zeros((mesh.mP + 1, n), dtype=np.int64)
    for i, el in enumerate(mesh.mElements):
        inds[:, i] = el.mNodesInd
    return inds


def dg_smoother(dgMesh, A, smootherType, ctx=None):
    """dg_smoother(mesh, A, :jac | :blockJac) src/smoother.jl:142-168"""
    if smootherType == 'jac':
        return JacobiSmoother(A, ctx)
    if smootherType == 'blockJac':
        return BlockJacobi(A, _mesh_block_inds(dgMesh), ctx)
    if smootherType == 'blockGS':    # extension, see BlockGaussSeidel
        return BlockGaussSeidel(A, _mesh_block_inds(dgMesh), ctx)
    if smootherType == 'patchSchwarz':    # extension, see ElementPatchSchwarz: hybrid patches of two elements
        m, ne = _mesh_block_inds(dgMesh).shape
        return ElementPatchSchwarz(A, m, ne, ctx=ctx)
    if smootherType == 'patchGS':    # extension, see ElementPatchGaussSeidel: multiplicative patches of two elements
        m, ne = _mesh_block_inds(dgMesh).shape
        return ElementPatchGaussSeidel(A, m, ne, ctx=ctx)
    raise ArgumentError(f"dg_smoother: unknown smoother type {smootherType!r}")


def cg_smoother(cgMesh, A, smootherType, ctx=None):
    """cg_smoother(mesh, A, :jac | :addSchwarz | :hybridSchwarz) src/smoother.jl:88-139"""
    if smootherType == 'jac':
        has_elements = cgMesh is not None and (hasattr(cgMesh, "mBlockInds") or hasattr(cgMesh, "mElements"))
        return JacobiSmoother(A, ctx, _mesh_block_inds(cgMesh) if has_elements else None)
    if smootherType == 'addSchwarz':
        return AdditiveSchwarzSmoother(A, _mesh_block_inds(cgMesh), ctx)
    if smootherType == 'hybridSchwarz':
        return HybridSchwarzSmoother(A, _mesh_block_inds(cgMesh), ctx)
    if smootherType == 'blockGS':    # extension: red-black ELEMENT Gauss-Seidel on the element chain, see BlockGaussSeidel
        return BlockGaussSeidel(A, _mesh_block_inds(cgMesh), ctx)
    raise ArgumentError(f"cg_smoother: unknown smoother type {smootherType!r}")


def apply_smoother(S, B, alpha=1.0):
    """apply_smoother(A::AbstractSmoother, B::AbstractVecOrMat; alpha=1.0) -> new array
    (src/smoother.jl:6,30,56,69).  B is not modified."""
    B = np.asarray(B, dtype=np.float64)
    if B.ndim not in (1, 2):
        raise DimensionMismatch("apply_smoother: B must be a vector or a matrix")
    N = B.shape[0]
    ncols = 1 if B.ndim == 1 else B.shape[1]
    Bf = np.asfortranarray(B.reshape(N, ncols))
    Y = np.empty((N, ncols), order='F')
    c = S.A.ctx
    c.check(c.lib.aggmg_smoother_apply(c.handle, S.handle, Bf.ctypes.data_as(_PD), N, ncols,
                                       float(alpha), Y.ctypes.data_as(_PD)))
    return Y[:, 0].copy() if B.ndim == 1 else np.ascontiguousarray(Y)


# --------------------------------------------------------------------------------------------
# hierarchy (src/mesh_heirarchy.jl) and solvers (src/solvers.jl)
# --------------------------------------------------------------------------------------------
def _is_cg_mesh(mesh):
    """a CgMesh shares vertices between elements (src/cg_mesh.jl:37-45): n p + 1 nodes on n elements"""
    try:
        els = mesh.mElements
        return mesh.mNumNodes == len(els) * mesh.mP + 1 and mesh.mP >= 1
    except AttributeError:
        return False


def _smoother_from_reference(S, A_op, mesh=None):
    """Accept the reference's smoother objects (anything with `mJac`, or `mBlockInds` [+
    `mCountingMatrix`]) as well as this module's; blocks are re-extracted from A on device.  A
    JacobiSmoother on a CG mesh also receives the mesh's element node lists (what
    cg_smoother(cgMesh, A, :jac) has at hand, src/smoother.jl:88-102)."""
    if isinstance(S, AbstractSmoother):
        return S
    if hasattr(S, "mCountingMatrix"):
        return HybridSchwarzSmoother(A_op, S.mBlockInds)
    if type(S).__name__ == "BlockGaussSeidelRB":     # the oracle's restatement of the extension
        return BlockGaussSeidel(A_op, S.mBlockInds)
    if hasattr(S, "mBlockInds"):
        return BlockJacobi(A_op, S.mBlockInds)
    if hasattr(S, "mJac"):
        if mesh is not None and _is_cg_mesh(mesh):
            return JacobiSmoother(A_op, None, _mesh_block_inds(mesh))
        return JacobiSmoother(A_op)
    raise ArgumentError("unrecognised smoother object")


class MeshHierarchy:
    """struct MeshHierarchy (src/mesh_heirarchy.jl:17-28) with device mirrors of the operator
    vectors.  Fields keep the reference's names; level 1 (index 0) is the finest.

    MeshHierarchy(mMeshes, mStiffness, mSmoothers, mInterpolation, mBdConds=None, ...) is the
    struct's positional constructor (the reference's two outer constructors do Galerkin set-up,
    which is outside the hot path: SURVEY.md 8 a12/a13); `from_reference(H)` wraps any object
    carrying the reference's fields (e.g. the set-up output of a Julia-side or oracle-side
    constructor)."""

    def __init__(self, mMeshes, mStiffness, mSmoothers, mInterpolation, mBdConds=None,
                 mGradient=None, mDivergence=None, mC=None, ctx=None, keep_host=True,
                 coarse_mode=_lib.COARSE_AUTO):
        n = len(mStiffness)
        if n < 1:
            raise ArgumentError("At least one mesh required.")
        if mMeshes is not None and len(mMeshes) != n:
            raise ArgumentError("Length of vector of meshes does not match the operators.")
        if len(mInterpolation) != n - 1 or len(mSmoothers) < n - 1:
            raise ArgumentError("Need one interpolation and one smoother per non-coarsest level.")
        self.ctx = ctx or default_context()
        self.mMeshes = mMeshes
        self.mStiffness = list(mStiffness)
        self.mInterpolation = list(mInterpolation)
        self.mBdConds = mBdConds
        self.mGradient, self.mDivergence, self.mC = mGradient, mDivergence, mC
        self._ops = [_as_op(A, _lib.OP_STIFFNESS, self.ctx) for A in mStiffness]
        self._Ls = [_as_op(L, _lib.OP_TRANSFER, self.ctx) for L in mInterpolation]
        self.mSmoothers = [_smoother_from_reference(mSmoothers[k], self._ops[k],
                                                    mMeshes[k] if mMeshes is not None else None)
                           for k in range(n - 1)]
        arr = ctypes.c_void_p * n
        ops = arr(*[o.handle for o in self._ops])
        sms = arr(*([s.handle for s in self.mSmoothers] + [None]))
        Ls = arr(*([l.handle for l in self._Ls] + [None]))
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.aggmg_hier_create(self.ctx.handle, n, ops, sms, Ls, int(coarse_mode), ctypes.byref(h)))
        self.handle = h
        if not keep_host:
            for o in self._ops + self._Ls:
                o.release_host()

    @classmethod
    def from_reference(cls, H, ctx=None, coarse_mode=_lib.COARSE_AUTO):
        return cls(H.mMeshes, H.mStiffness, H.mSmoothers, H.mInterpolation,
                   getattr(H, "mBdConds", None), getattr(H, "mGradient", None),
                   getattr(H, "mDivergence", None), getattr(H, "mC", None), ctx=ctx,
                   coarse_mode=coarse_mode)

    @classmethod
    def from_dg_operators(cls, mMeshes, A, G, D, C, mInterpolation, mMassMatrices, ctx=None, keep_host=True,
                          coarse_mode=_lib.COARSE_AUTO, smoothers='blockJac'):
        """MeshHierarchy(mMeshes, mBdConds, A, G, D, C; nDG, nAgg) (src/mesh_heirarchy.jl:140-181, with the
        agglomerated levels of SURVEY D4) given the interpolation matrices L_k and the mass matrices
        (BlockDiagonal) of the coarser levels: the recurrences of :79-84 / :98-103 run on the device --

            G_{k+1} = L' * G_k * L,  D_{k+1} = L' * D_k * L,  C_{k+1} = L' * C_k * L
            A_{k+1} = C_{k+1} - D_{k+1} * (M_LU \\ G_{k+1})
            mSmoothers[k] = dg_smoother(mMeshes[k], A_k, :blockJac)

        (aggmg_op_transpose, aggmg_sp_matmul, aggmg_bd_sp_apply, aggmg_sp_sub, aggmg_blockjacobi_setup).
        mMeshes[k] need `mBlockInds` (or `mElements` / `mP`); mMassMatrices[k] is the BlockDiagonal of
        level k + 1.  The Galerkin operators stay in HBM; H.mGradient / mDivergence / mC / mStiffness hold
        DeviceOperators (`.to_scipy()` reads one back).
        smoothers: the dg_smoother type of every smoothed level, or a list of one per level ('blockJac', the
        reference's; 'patchSchwarz', 'patchGS', 'blockGS', 'jac': extensions / other reference types)."""
        ctx = ctx or default_context()
        n = len(mMeshes)
        if n < 1:
            raise ArgumentError("At least one DG mesh required.")
        kinds = [smoothers] * (n - 1) if isinstance(smoothers, str) else list(smoothers)
        if len(kinds) != n - 1:
            raise ArgumentError("smoothers: one smoother type per non-coarsest level")
        if len(mInterpolation) != n - 1 or len(mMassMatrices) != n - 1:
            raise ArgumentError("Length of vector of meshes does not match inputed number of DG and "
                                "agglomerated meshes.")
        St = [_as_op(A, _lib.OP_STIFFNESS, ctx)]
        Gs, Ds, Cs = [_as_op(G, _lib.OP_STIFFNESS, ctx)], [_as_op(D, _lib.OP_STIFFNESS, ctx)], [_as_op(C, _lib.OP_STIFFNESS, ctx)]
        Ls = [_as_op(L, _lib.OP_TRANSFER, ctx) for L in mInterpolation]
        for k in range(n - 1):
            L = Ls[k]
            Lt = L.transpose()
            Gs.append(Lt.matmul(Gs[k]).matmul(L))         # (L' * G) * L, left to right as Julia evaluates it
            Ds.append(Lt.matmul(Ds[k]).matmul(L))
            Cs.append(Lt.matmul(Cs[k]).matmul(L))
            M = mMassMatrices[k]
            Mlu = M if isinstance(M, BlockDiagonalLU) else M.lu()
            St.append(Cs[k + 1].sub(Ds[k + 1].matmul(Mlu.solve(Gs[k + 1]))))
            Lt.free()
        sms = [dg_smoother(mMeshes[k], St[k], kinds[k], ctx) for k in range(n - 1)]
        H = cls(mMeshes, St, sms, Ls, mGradient=Gs, mDivergence=Ds, mC=Cs, ctx=ctx, keep_host=keep_host,
                coarse_mode=coarse_mode)
        return H

    @classmethod
    def from_cg_operators(cls, mMeshes, A, mInterpolation, nCG, dg_operators=None, mMassMatrices=(), ctx=None,
                          keep_host=True, coarse_mode=_lib.COARSE_AUTO):
        """MeshHierarchy(mMeshes, mesh, mBdConds, A; nCG, nDG, nAgg, CDir) (src/mesh_heirarchy.jl:30-138) given
        the interpolation matrices of all levels: the CG chain's Galerkin operators `L'*A*L` (:53-59) and, below
        the first DG / agglomerated level, the recurrences of :76-86 / :89-106 run on the device.  That first
        DG level is RE-DISCRETISED in the reference (:65-72, dg_flux_operators -- assembly, outside the hot path):
        its G, D, C come in through dg_operators = (G, D, C); mMassMatrices[i] is the BlockDiagonal mass matrix
        of level nCG + i.  CG levels get cg_smoother(mesh, A, :jac) with the mesh's element lists, DG levels
        dg_smoother(mesh, A, :blockJac)."""
        ctx = ctx or default_context()
        n = len(mMeshes)
        if nCG <= 0:
            raise ArgumentError("At least one CG mesh required.")
        if len(mInterpolation) != n - 1 or (n > nCG and (dg_operators is None or len(mMassMatrices) != n - nCG)):
            raise ArgumentError("Length of vector of meshes does not match inputed number of CG, DG, and "
                                "agglomerated meshes.")
        Ls = [_as_op(L, _lib.OP_TRANSFER, ctx) for L in mInterpolation]
        St = [_as_op(A, _lib.OP_STIFFNESS, ctx)]
        for i in range(nCG - 1):
            Lt = Ls[i].transpose()
            St.append(Lt.matmul(St[i]).matmul(Ls[i]))
            Lt.free()
        Gs, Ds, Cs = [], [], []
        if n > nCG:
            Gs.append(_as_op(dg_operators[0], _lib.OP_STIFFNESS, ctx))
            Ds.append(_as_op(dg_operators[1], _lib.OP_STIFFNESS, ctx))
            Cs.append(_as_op(dg_operators[2], _lib.OP_STIFFNESS, ctx))
            lus = [M if isinstance(M, BlockDiagonalLU) else M.lu() for M in mMassMatrices]
            St.append(Cs[0].sub(Ds[0].matmul(lus[0].solve(Gs[0]))))
            for i in range(1, n - nCG):
                L = Ls[nCG + i - 1]
                Lt = L.transpose()
                Gs.append(Lt.matmul(Gs[i - 1]).matmul(L))
                Ds.append(Lt.matmul(Ds[i - 1]).matmul(L))
                Cs.append(Lt.matmul(Cs[i - 1]).matmul(L))
                St.append(Cs[i].sub(Ds[i].matmul(lus[i].solve(Gs[i]))))
                Lt.free()
        sms = []
        for k in range(n - 1):
            if k < nCG:
                sms.append(cg_smoother(mMeshes[k], St[k], 'jac', ctx))
            else:
                sms.append(BlockJacobi(St[k], _mesh_block_inds(mMeshes[k]), ctx))
        return cls(mMeshes, St, sms, Ls, mGradient=Gs, mDivergence=Ds, mC=Cs, ctx=ctx, keep_host=keep_host,
                   coarse_mode=coarse_mode)

    @property
    def nlevels(self):
        return len(self._ops)

    def structured_levels(self):
        return [s.structured for s in self.mSmoothers]

    def level_kinds(self):
        """which kernels run each level: 'fused_btd', 'fused_chain', 'generic', 'coarsest' (C ABI
        aggmg_hier_level_kind)"""
        out = []
        for k in range(self.nlevels):
            v = ctypes.c_int(0)
            self.ctx.check(self.ctx.lib.aggmg_hier_level_kind(self.ctx.handle, self.handle, k, ctypes.byref(v)))
            out.append(_lib.LEVEL_KIND_NAMES[v.value])
        return out

    def sym_residual_levels(self):
        """levels whose explicit residual reads the lossless symmetric form of the operator's entries (C ABI
        aggmg_hier_level_sym_residual, AGGMG_OPT_SYMMETRIC_RESIDUAL)"""
        out = []
        for k in range(self.nlevels):
            v = ctypes.c_int(0)
            self.ctx.check(self.ctx.lib.aggmg_hier_level_sym_residual(self.ctx.handle, self.handle, k, ctypes.byref(v)))
            if v.value:
                out.append(k)
        return out

    def dictionary_levels(self):
        """{level: distinct operator records} of the levels whose cycle launches index the operator through a
        dictionary of its distinct per-element records (C ABI aggmg_hier_level_dictionary,
        AGGMG_OPT_OPERATOR_DICTIONARY)"""
        out = {}
        for k in range(self.nlevels):
            v = ctypes.c_int(0)
            self.ctx.check(self.ctx.lib.aggmg_hier_level_dictionary(self.ctx.handle, self.handle, k, ctypes.byref(v)))
            if v.value:
                out[k] = v.value
        return out

    def patch_dictionary_levels(self):
        """{level: distinct operator records} of the levels whose fused element-patch Schwarz smoother sweeps through
        a dictionary of its own (ElementPatchSchwarz / ElementPatchGaussSeidel.dictionary_classes, C ABI
        aggmg_smoother_patch_dictionary)"""
        out = {}
        for k, S in enumerate(self.mSmoothers):
            nc = getattr(S, "dictionary_classes", 0)
            if nc:
                out[k] = nc
        return out

    def paired_levels(self, nsweeps=3, direction="down"):
        """levels k whose launch also carries level k + 1 (C ABI aggmg_hier_level_paired / _paired_up), as the descent
        walks the hierarchy (pairs taken from the fine side) or, direction='up', as the ascent does (from the coarse
        side); the two directions have tiles of their own and may differ"""
        fn = self.ctx.lib.aggmg_hier_level_paired if direction == "down" else self.ctx.lib.aggmg_hier_level_paired_up

        def ok(k):
            v = ctypes.c_int(0)
            self.ctx.check(fn(self.ctx.handle, self.handle, k, int(nsweeps), ctypes.byref(v)))
            return bool(v.value)
        out = []
        if direction == "down":
            k = 0
            while k < self.nlevels - 1:
                if ok(k):
                    out.append(k)
                    k += 1
                k += 1
        else:
            k = self.nlevels - 2
            while k >= 1:
                if ok(k - 1):
                    out.append(k - 1)
                    k -= 1
                k -= 1
        return sorted(out)

    def launch_bytes(self, level, kind, has_x0=None):
        """(read, write) compulsory HBM bytes of the fused launch of `level`: kind 'down' / 'up' / 'mid'
        (C ABI aggmg_hier_launch_bytes) -- every array of the launch counted once, as stored.  'down' and 'up' are the
        launches that store the pre-smoothed iterate and read it back; 'replay_down' / 'replay_up' those of a cycle
        that replays its pre-smoothing (AGGMG_OPT_REPLAY_PRESMOOTH)."""
        kk = {"down": _lib.KIND_FUSED_DOWN, "up": _lib.KIND_FUSED_UP, "mid": _lib.KIND_FUSED_MID,
              "replay_down": _lib.KIND_REPLAY_DOWN, "replay_up": _lib.KIND_REPLAY_UP}[kind]
        r, w = ctypes.c_int64(0), ctypes.c_int64(0)
        x0 = (level == 0) if has_x0 is None else bool(has_x0)
        self.ctx.check(self.ctx.lib.aggmg_hier_launch_bytes(self.ctx.handle, self.handle, int(level), kk, int(x0),
                                                            ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def vcycle_dev(self, x0, b, x_out, nPre=3, nPost=3, alpha=2.0 / 3.0):
        """Device-resident V-cycle: x0, b, x_out are DeviceVector / torch tensors / raw pointers;
        asynchronous on the context stream."""
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_dev(c.handle, self.handle, _ptr(x0), _ptr(b), int(nPre), int(nPost),
                                       float(alpha), _ptr(x_out)))

    def vcycle_multi_dev(self, X0, B, X, ncols=None, ld=None, nPre=3, nPost=3, alpha=2.0 / 3.0):
        """Device-resident V-cycle on K right-hand sides (C ABI aggmg_vcycle_multi_dev; EXTENSION): X0 (None: zero
        guesses), B, X are DeviceMatrix / column-major device buffers with leading dimension ld (default N); column j of
        X is bit for bit vcycle_dev of column j.  Asynchronous on the context stream."""
        N = self._ops[0].shape[0]
        if ncols is None:
            ncols = B.k if isinstance(B, DeviceMatrix) else None
        if ncols is None:
            raise ArgumentError("vcycle_multi_dev: ncols is needed for raw device pointers")
        if ld is None:
            ld = N
        for M_ in (X0, B, X):   # (ncols < 1, ld < N: the C ABI's ArgumentError)
            if isinstance(M_, DeviceMatrix) and int(ncols) >= 1 and (M_.n != N or M_.k < int(ncols)):
                raise DimensionMismatch("vcycle_multi_dev: matrix shape does not match (N, ncols)")
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_multi_dev(c.handle, self.handle, _ptr(X0), _ptr(B), int(ncols), int(ld), int(nPre),
                                             int(nPost), float(alpha), _ptr(X)))

    def coarse_solve_multi_dev(self, B, X, ncols=None, ld=None):
        """X = A_n \\ B, the coarsest-level direct solve (src/solvers.jl:39) on K right-hand sides, resident on the device
        (C ABI aggmg_hier_coarse_solve_multi_dev; EXTENSION) -- for a one-level hierarchy the `A \\ B` of :120.  B, X:
        DeviceMatrix / column-major device buffers of N_n rows (the coarsest operator's) with leading dimension ld
        (default N_n); on the device factorisation a group of columns shares every launch and column j of X is bit for
        bit the single-column solve of column j.  Asynchronous on the context stream."""
        N = self._ops[-1].shape[0]
        for M_ in (B, X):
            if isinstance(M_, np.ndarray) or M_ is None:
                raise ArgumentError("coarse_solve_multi_dev: B and X must be DeviceMatrix objects or device buffers")
        if ncols is None:
            ncols = B.k if isinstance(B, DeviceMatrix) else None
        if ncols is None:
            raise ArgumentError("coarse_solve_multi_dev: ncols is needed for raw device pointers")
        if ld is None:
            ld = N
        for M_ in (B, X):   # (ncols < 1, ld < N: the C ABI's ArgumentError)
            if isinstance(M_, DeviceMatrix) and int(ncols) >= 1 and (M_.n != N or M_.k < int(ncols)):
                raise DimensionMismatch("coarse_solve_multi_dev: matrix shape does not match (N, ncols)")
        c = self.ctx
        c.check(c.lib.aggmg_hier_coarse_solve_multi_dev(c.handle, self.handle, _ptr(B), int(ncols), int(ld), _ptr(X)))

    def pcg_multi_dev(self, B, X, ncols=None, ld=None, maxiter=50, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0):
        """pcg on K right-hand sides, resident on the device (C ABI aggmg_pcg_multi_dev; EXTENSION): B, X (initial guesses
        in, results out) DeviceMatrix / column-major device buffers.  -> (iters[K], res: K lists, work_cols)"""
        N = self._ops[0].shape[0]
        _, K, ld = _cols_shape("pcg_multi_dev", B, N, ncols, ld)
        hist = np.zeros((max(1, K), max(1, int(maxiter))))
        its = np.zeros(max(1, K), dtype=np.int32)
        work = ctypes.c_int64(0)
        c = self.ctx
        c.check(c.lib.aggmg_pcg_multi_dev(c.handle, self.handle, _ptr(B), _ptr(X), K, ld, int(maxiter), float(tol), int(nPre),
                                          int(nPost), float(alpha), _pd(hist), its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                          ctypes.byref(work)))
        return its[:K].copy(), [hist[j, :its[j]].tolist() for j in range(K)], work.value

    def fgmres_multi_dev(self, B, X, ncols=None, ld=None, restart=30, maxiter=200, tol=1e-10, nPre=3, nPost=3,
                         alpha=2.0 / 3.0):
        """fgmres on K right-hand sides in lockstep, resident on the device (C ABI aggmg_fgmres_multi_dev; EXTENSION): B,
        X (initial guesses in, results out) DeviceMatrix / column-major device buffers.  Column j is bit for bit
        aggmg_fgmres_dev on column j.  -> (iters[K], res: K lists, work_cols)"""
        N = self._ops[0].shape[0]
        _, K, ld = _cols_shape("fgmres_multi_dev", B, N, ncols, ld)
        hist = np.zeros((max(1, K), max(1, int(maxiter))))
        its = np.zeros(max(1, K), dtype=np.int32)
        work = ctypes.c_int64(0)
        c = self.ctx
        c.check(c.lib.aggmg_fgmres_multi_dev(c.handle, self.handle, _ptr(B), _ptr(X), K, ld, int(restart), int(maxiter),
                                             float(tol), int(nPre), int(nPost), float(alpha), _pd(hist),
                                             its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(work)))
        return its[:K].copy(), [hist[j, :its[j]].tolist() for j in range(K)], work.value

    def multigrid_multi_dev(self, X0, B, X, maxiter, tol, ncols=None, ld=None, check_every=1, nPre=3, nPost=3, alpha=2.0 / 3.0,
                            U_exact=None):
        """multigrid on K right-hand sides, resident on the device (C ABI aggmg_multigrid_multi_dev; EXTENSION): X0, B, X
        (and U_exact, the fine-level direct solutions, or None) DeviceMatrix / column-major device buffers.
        -> (cycles[K], res: K lists, err: K lists ([] each without U_exact), work_cols)"""
        N = self._ops[0].shape[0]
        _, K, ld = _cols_shape("multigrid_multi_dev", B, N, ncols, ld)
        nchk = max(1, -(-int(maxiter) // max(1, int(check_every))))
        hist, ehist = np.zeros((max(1, K), nchk)), np.zeros((max(1, K), nchk))
        ncyc, nck = np.zeros(max(1, K), dtype=np.int32), np.zeros(max(1, K), dtype=np.int32)
        work = ctypes.c_int64(0)
        pi = ctypes.POINTER(ctypes.c_int)
        c = self.ctx
        c.check(c.lib.aggmg_multigrid_multi_dev(c.handle, self.handle, _ptr(X0), _ptr(B), K, ld, int(maxiter), float(tol),
                                                int(check_every), int(nPre), int(nPost), float(alpha), _ptr(X), _pd(hist),
                                                ncyc.ctypes.data_as(pi), nck.ctypes.data_as(pi), _ptr(U_exact),
                                                _pd(ehist) if U_exact is not None else None, ctypes.byref(work)))
        res = [hist[j, :nck[j]].tolist() for j in range(K)]
        err = [ehist[j, :nck[j]].tolist() if U_exact is not None else [] for j in range(K)]
        return ncyc[:K].copy(), res, err, work.value

    def multi_info(self, K, nPre=3, nPost=3):
        """-> (fused, group): whether a K-column cycle runs K-column launches (True) or the single-column cycle column by
        column (False), and the columns per launch (C ABI aggmg_hier_multi_info)"""
        f, g = ctypes.c_int(0), ctypes.c_int(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_multi_info(self.ctx.handle, self.handle, int(K), int(nPre), int(nPost),
                                                          ctypes.byref(f), ctypes.byref(g)))
        return bool(f.value), g.value

    def multi_element_thread_levels(self, nPre=3, nPost=3):
        """{level: (down, up)}: the levels of a K-column V(nPre, nPost) cycle with a half that the K-column element-thread
        kernel would serve under the context's options as they stand, and which halves (C ABI
        aggmg_hier_level_multi_element_threads, AGGMG_OPT_MULTI_ELEMENT_THREADS)"""
        out = {}
        for k in range(len(self._ops)):
            d, u = ctypes.c_int(0), ctypes.c_int(0)
            self.ctx.check(self.ctx.lib.aggmg_hier_level_multi_element_threads(self.ctx.handle, self.handle, k, int(nPre), int(nPost),
                                                                               ctypes.byref(d), ctypes.byref(u)))
            if d.value or u.value:
                out[k] = (bool(d.value), bool(u.value))
        return out

    def multi_launch_bytes(self, level, kind, K, has_x0=None):
        """(read, write) compulsory HBM bytes of a K-column fused launch of `level`, kind 'down' / 'up' (C ABI
        aggmg_hier_multi_launch_bytes): the operator's arrays once, the vectors once per column"""
        kk = {"down": _lib.KIND_FUSED_DOWN, "up": _lib.KIND_FUSED_UP}[kind]
        r, w = ctypes.c_int64(0), ctypes.c_int64(0)
        x0 = (level == 0) if has_x0 is None else bool(has_x0)
        self.ctx.check(self.ctx.lib.aggmg_hier_multi_launch_bytes(self.ctx.handle, self.handle, int(level), kk, int(x0),
                                                                  int(K), ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def vcycles_dev(self, x0, b, x_out, ncycles, nPre=3, nPost=3, alpha=2.0 / 3.0):
        """ncycles device-resident V-cycles back to back (x <- V(x, b)), the loop body of
        multigrid (src/solvers.jl:124-126); between cycles the fine level's post- and pre-smoothing
        share one fused launch."""
        c = self.ctx
        c.check(c.lib.aggmg_vcycles_dev(c.handle, self.handle, _ptr(x0), _ptr(b), int(ncycles), int(nPre),
                                        int(nPost), float(alpha), _ptr(x_out)))

    def vcycle_down_dev(self, x0, b, nPre=3, alpha=2.0 / 3.0):
        """Descending half (src/solvers.jl:28-37); leaves the coarsest rhs in coarse_buffers()."""
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_down_dev(c.handle, self.handle, _ptr(x0), _ptr(b), int(nPre), float(alpha)))

    def vcycle_up_dev(self, b, x_out, nPost=3, alpha=2.0 / 3.0):
        """Ascending half (src/solvers.jl:41-47); the coarsest solution must be in coarse_buffers()."""
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_up_dev(c.handle, self.handle, _ptr(b), int(nPost), float(alpha), _ptr(x_out)))

    def vcycle_up_split_dev(self, b, x_out, head_elems, tail_elem, part, nPost=3, alpha=2.0 / 3.0):
        """the ascent in three calls (C ABI aggmg_vcycle_up_split_dev): part 0 = coarser levels, part 1 =
        the fine-level tiles holding elements [0, head_elems) and [tail_elem, ne), part 2 = the rest"""
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_up_split_dev(c.handle, self.handle, _ptr(b), int(nPost), float(alpha), _ptr(x_out),
                                                int(head_elems), int(tail_elem), int(part)))

    def can_split_up(self, nPost=3):
        """whether parts 0 - 2 of vcycle_up_split_dev exist for this hierarchy and sweep count (C ABI
        aggmg_vcycle_up_split_ok): a fused block-tridiagonal fine level, or a multiplicative element-patch level with a
        one-ratio transfer and 1 <= nPost <= the sweeps of one launch"""
        ok = ctypes.c_int(0)
        c = self.ctx
        c.check(c.lib.aggmg_vcycle_up_split_ok(c.handle, self.handle, int(nPost), ctypes.byref(ok)))
        return bool(ok.value)

    def set_restriction(self, mode):
        """_lib.RESTRICT_EXPLICIT (default: the reference's arithmetic for L'(rhs - A u)) or
        _lib.RESTRICT_PRECONDITIONED (cheaper; UnsupportedError above
        _lib.RESTRICT_PRECONDITIONED_MAX_ELEMS fine elements, where its rounding error on the smoothest
        mode would stall or reverse convergence) -- C ABI aggmg_hier_set_restriction, include/aggmg_hip.h"""
        c = self.ctx
        c.check(c.lib.aggmg_hier_set_restriction(c.handle, self.handle, int(mode)))

    # ---- sweep-weight schedules (EXTENSION: the reference damps every sweep of every level by the same alpha) ----
    def set_sweep_weights(self, level, pre, post=None):
        """Level `level` damps its i-th pre-smoothing sweep by pre[i] and its i-th post-smoothing sweep by post[i] in every
        solver that runs the cycle on this hierarchy (vcycle, vcycles, multigrid, pcg, their K-column forms), in place of
        their `alpha`; levels without a schedule keep `alpha` (C ABI aggmg_hier_set_sweep_weights).  post defaults to pre
        reversed, which keeps the cycle a symmetric preconditioner for pcg; with an explicit post that is not pre
        reversed, symmetry is the caller's responsibility.  A cycle's nPre / nPost must equal len(pre) / len(post)
        (ArgumentError otherwise); at most _lib.MAX_SWEEP_WEIGHTS weights per half, all finite; the coarsest level has no
        sweeps."""
        pre = np.ascontiguousarray(np.atleast_1d(np.asarray(pre, dtype=np.float64)))
        post = pre[::-1].copy() if post is None else np.ascontiguousarray(np.atleast_1d(np.asarray(post, dtype=np.float64)))
        if pre.ndim != 1 or post.ndim != 1:
            raise ArgumentError("set_sweep_weights: pre and post are sequences of numbers")
        c = self.ctx
        c.check(c.lib.aggmg_hier_set_sweep_weights(c.handle, self.handle, int(level), _pd(pre), pre.size, _pd(post), post.size))

    def clear_sweep_weights(self, level=None):
        """remove the schedule of `level`, or (None) of every level: the cycle is the entry point's `alpha` again"""
        c = self.ctx
        for k in (range(self.nlevels - 1) if level is None else [int(level)]):
            c.check(c.lib.aggmg_hier_set_sweep_weights(c.handle, self.handle, k, None, 0, None, 0))

    def sweep_weights(self, level):
        """-> (pre, post) arrays of the level's schedule, or None when it has none (C ABI aggmg_hier_get_sweep_weights)"""
        pre, post = np.zeros(_lib.MAX_SWEEP_WEIGHTS), np.zeros(_lib.MAX_SWEEP_WEIGHTS)
        npre, npost = ctypes.c_int(0), ctypes.c_int(0)
        c = self.ctx
        c.check(c.lib.aggmg_hier_get_sweep_weights(c.handle, self.handle, int(level), _pd(pre), ctypes.byref(npre), _pd(post),
                                                   ctypes.byref(npost)))
        if npre.value + npost.value == 0:
            return None
        return pre[:npre.value].copy(), post[:npost.value].copy()

    def estimate_lambda_max(self, level, iters=40, v0=None):
        """largest eigenvalue of S^-1 A of `level` by `iters` steps of power iteration on the device, one host read at the
        end (C ABI aggmg_hier_estimate_lambda_max).  v0: start vector (host array, DeviceVector, tensor or pointer), or
        None for a fixed seeded one.  The estimate approaches the eigenvalue from below."""
        c = self.ctx
        keep = None
        if v0 is not None and isinstance(v0, (np.ndarray, list, tuple)):
            keep = c.to_device(v0)
            v0 = keep
        lam = ctypes.c_double(0.0)
        try:
            c.check(c.lib.aggmg_hier_estimate_lambda_max(c.handle, self.handle, int(level), None if v0 is None else _ptr(v0),
                                                         int(iters), ctypes.byref(lam)))
        finally:
            if keep is not None:
                keep.free()
        return lam.value

    def set_chebyshev_smoothing(self, levels=(0,), degree=3, ratio=10.0, iters=40):
        """estimate_lambda_max on each of `levels`, then chebyshev_weights(lam, degree, ratio) as the level's pre-smoothing
        schedule and its reverse as the post-smoothing one; -> {level: lambda_max estimate}.  The cycle then runs with
        nPre = nPost = degree."""
        out = {}
        for k in levels:
            lam = self.estimate_lambda_max(k, iters=iters)
            self.set_sweep_weights(k, chebyshev_weights(lam, degree=degree, ratio=ratio))
            out[int(k)] = lam
        return out

    def get_restriction(self):
        v = ctypes.c_int(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_get_restriction(self.ctx.handle, self.handle, ctypes.byref(v)))
        return v.value

    def coarse_buffers(self):
        """-> (rhs_ptr, sol_ptr, n): device buffers of the coarsest level"""
        r, s_, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_buffers(self.ctx.handle, self.handle, ctypes.byref(r),
                                                              ctypes.byref(s_), ctypes.byref(n)))
        return r.value, s_.value, n.value

    def coarse_info(self):
        """-> dict(on_device, block_size, cond_est, probe_backward_error, tail, tail_blocks, order) of the coarsest direct
        solver; probe_backward_error: ||d - A x|| / ||d|| of the probe solve that aggmg_hier_create accepts (< 1e-10) or
        rejects the device factorisation on (-1: none attempted); order: "operator" -- the blocks are the operator's own
        rows -- or "element chain" (COARSE_DEVICE_CHAIN; COARSE_AUTO where the host solver refuses the band): block_size
        is then the degree p of the CG operator"""
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0.0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_info(self.ctx.handle, self.handle, ctypes.byref(a),
                                                           ctypes.byref(b), ctypes.byref(c)))
        e = ctypes.c_double(0.0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_probe(self.ctx.handle, self.handle, ctypes.byref(e)))
        k, nb = ctypes.c_int(0), ctypes.c_int64(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_tail(self.ctx.handle, self.handle, ctypes.byref(k), ctypes.byref(nb)))
        on, cm, cb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_chain(self.ctx.handle, self.handle, ctypes.byref(on), ctypes.byref(cm),
                                                            ctypes.byref(cb)))
        return dict(on_device=bool(a.value), block_size=b.value, cond_est=c.value, probe_backward_error=e.value,
                    tail=("none", "cyclic reduction", "parallel cyclic reduction")[k.value], tail_blocks=nb.value,
                    order="element chain" if on.value else "operator")

    def coarse_dictionary(self):
        """-> dict(stages=[dict(taken, first_level, levels)], even_classes=[...], odd_classes=[...]) of the coarsest
        solve's dictionary (AGGMG_OPT_COARSE_DICTIONARY; C ABI aggmg_hier_coarse_dictionary): per chunk stage whether its
        launches read their factors from LDS and the reducing levels it spans; per reducing level up to the last one of
        the last stage the distinct records among its even rows' multipliers and among its odd rows' factors (-1: not
        classed, 0: more than the search tracks)"""
        cap = 64
        arr = [(ctypes.c_int * cap)() for _ in range(5)]
        ns = ctypes.c_int(0)
        self.ctx.check(self.ctx.lib.aggmg_hier_coarse_dictionary(self.ctx.handle, self.handle, cap, ctypes.byref(ns), *arr))
        taken, first, nlv, ev, od = arr
        stages = [dict(taken=bool(taken[s]), first_level=int(first[s]), levels=int(nlv[s])) for s in range(ns.value)]
        nl = max((s["first_level"] + s["levels"] for s in stages), default=0)
        return dict(stages=stages, even_classes=[int(ev[l]) for l in range(nl)], odd_classes=[int(od[l]) for l in range(nl)])

    def last_coarse_ms(self):
        ms = ctypes.c_double(0.0)
        self.ctx.check(self.ctx.lib.aggmg_hier_last_coarse_ms(self.ctx.handle, self.handle, ctypes.byref(ms)))
        return ms.value

    def free(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.lib.aggmg_hier_free(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def multigrid_v_cycle(H, x0, b, nPre=3, nPost=3, alpha=2.0 / 3.0, out=None):
    """multigrid_v_cycle(H, x0, b; nPre=3, nPost=3, alpha=2/3) -> x   (src/solvers.jl:19-50).
    Returns a new vector; x0 and b are not modified.  x0, b: host arrays (-> NumPy array) or DeviceVectors
    (-> DeviceVector, nothing leaves the device).  out (host arrays only, an extension): the array the result goes to
    instead of a new one -- with x0, b, out page-locked once (Context.pin / pinned_empty) a call moves its three vectors
    by DMA instead of staging them."""
    if not isinstance(nPre, (int, np.integer)) or not isinstance(nPost, (int, np.integer)):
        raise TypeError("nPre / nPost must be integers (nPre::Integer, src/solvers.jl:20)")
    if isinstance(b, DeviceMatrix) or (not isinstance(b, DeviceVector) and np.ndim(b) == 2):
        return _multigrid_v_cycle_multi(H, x0, b, int(nPre), int(nPost), float(alpha))
    if x0 is None and isinstance(b, DeviceVector):      # zero initial guess (ldiv!): nothing is read for it
        out = H.ctx.alloc(b.n)
        H.vcycle_dev(None, b, out, int(nPre), int(nPost), float(alpha))
        return out
    if isinstance(x0, DeviceVector) and isinstance(b, DeviceVector):
        # vectors already in HBM: nothing crosses PCIe, a new DeviceVector comes back (aggmg_vcycle_dev) -- the form
        # for callers that loop; host arrays cost 3 * 8 * N bytes of PCIe per call (bench.py: pcie_inclusive)
        N = H._ops[0].shape[0]
        if x0.n != N or b.n != N:
            raise DimensionMismatch("multigrid_v_cycle: x0 / b do not match the fine operator")
        out = H.ctx.alloc(N)
        H.vcycle_dev(x0, b, out, int(nPre), int(nPost), float(alpha))
        return out
    x0 = None if x0 is None else _f64(x0)     # None: a zero initial guess (what ldiv! uses), no vector of zeros sent
    b = _f64(b)
    N = H._ops[0].shape[0]
    if (x0 is not None and x0.shape != (N,)) or b.shape != (N,):
        raise DimensionMismatch("multigrid_v_cycle: x0 / b do not match the fine operator")
    if out is None:
        out = np.empty(N)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (N,) and out.flags["C_CONTIGUOUS"]):
        raise DimensionMismatch("multigrid_v_cycle: out must be a contiguous float64 array of the fine operator's size")
    elif (x0 is not None and np.shares_memory(out, x0)) or np.shares_memory(out, b):
        raise ArgumentError("multigrid_v_cycle: out must not alias x0 or b (they are not modified)")
    c = H.ctx
    c.check(c.lib.aggmg_vcycle(c.handle, H.handle, None if x0 is None else _pd(x0), _pd(b), int(nPre), int(nPost), float(alpha),
                               _pd(out)))
    return out


def _multigrid_v_cycle_multi(H, X0, B, nPre, nPost, alpha):
    """K right-hand sides (EXTENSION; the reference's methods take vectors, src/solvers.jl:19,63,84): B an (N, K) host
    array in either memory order (-> (N, K) array) or a DeviceMatrix (-> DeviceMatrix); X0 likewise, or None for zero
    guesses.  Column j is bit for bit the single-vector cycle of column j (aggmg_vcycle_multi_dev)."""
    N = H._ops[0].shape[0]
    c = H.ctx
    if isinstance(B, DeviceMatrix):
        if X0 is not None and not isinstance(X0, DeviceMatrix):
            raise ArgumentError("multigrid_v_cycle: X0 must be a DeviceMatrix (or None) when B is one")
        K = B.k
        if B.n != N or (X0 is not None and X0.shape != B.shape):
            raise DimensionMismatch("multigrid_v_cycle: X0 / B do not match (N, K) of the fine operator")
        X = DeviceMatrix(c, N, K)
        H.vcycle_multi_dev(X0, B, X, K, N, nPre, nPost, alpha)
        return X
    if isinstance(X0, (DeviceVector, DeviceMatrix)):
        raise ArgumentError("multigrid_v_cycle: X0 is on the device but B is a host array")
    B = np.asarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != N:
        raise DimensionMismatch(f"multigrid_v_cycle: B has shape {B.shape}, expected ({N}, K)")
    K = B.shape[1]
    if K < 1:
        raise ArgumentError("multigrid_v_cycle: B has no columns")
    if X0 is not None:
        X0 = np.asarray(X0, dtype=np.float64)
        if X0.shape != B.shape:
            raise DimensionMismatch(f"multigrid_v_cycle: X0 has shape {X0.shape}, B {B.shape}")
    dB = DeviceMatrix(c, N, K)
    dB.upload(B)
    dX0 = None
    if X0 is not None:
        dX0 = DeviceMatrix(c, N, K)
        dX0.upload(X0)
    dX = DeviceMatrix(c, N, K)
    H.vcycle_multi_dev(dX0, dB, dX, K, N, nPre, nPost, alpha)
    return dX.download()


def ldiv(*args):
    """ldiv!(H, b) -- overwrites b (src/solvers.jl:63-71);  ldiv!(y, H, b) (src/solvers.jl:84-92).
    One V-cycle from a zero initial guess."""
    if len(args) == 2:
        H, b = args
        y = b
    elif len(args) == 3:
        y, H, b = args
    else:
        raise TypeError("ldiv(H, b) or ldiv(y, H, b)")
    N = H._ops[0].shape[0]
    u0 = None        # zero initial guess: aggmg_vcycle(x0 = NULL), no vector of zeros crosses PCIe
    if isinstance(b, DeviceMatrix) or (not isinstance(b, DeviceVector) and np.ndim(b) == 2):
        # K right-hand sides (EXTENSION): ldiv!(Y, H, B) with matrices, one K-column cycle from zero guesses.  The
        # DeviceMatrix form writes Y on the device and needs a Y apart from B (ArgumentError otherwise)
        if isinstance(b, DeviceMatrix):
            if not isinstance(y, DeviceMatrix):
                raise ArgumentError("ldiv: Y must be a DeviceMatrix when B is one")
            if y.shape != b.shape or b.n != N:
                raise DimensionMismatch(f"ldiv: Y has shape {y.shape}, B {b.shape}, the fine operator {N} rows")
            H.vcycle_multi_dev(None, b, y, b.k, N)
            return None
        Y = _multigrid_v_cycle_multi(H, None, b, 3, 3, 2.0 / 3.0)
        if np.shape(y) != Y.shape:
            raise DimensionMismatch(f"ldiv: Y has shape {np.shape(y)}, B {Y.shape}")
        y[...] = Y
        return None
    direct = (y is not b and isinstance(y, np.ndarray) and y.dtype == np.float64 and y.shape == (N,) and y.flags["C_CONTIGUOUS"]
              and not np.shares_memory(y, np.asarray(b)))
    if direct:      # straight into y: with y and b page-locked (Context.pin) nothing is staged
        multigrid_v_cycle(H, u0, b, out=y)
    else:
        y[:] = multigrid_v_cycle(H, u0, b)
    return None


def _device_residual_norm(H_or_op, x, b):
    op = H_or_op
    r = np.empty(op.shape[0])
    c = op.ctx
    c.check(c.lib.aggmg_residual(c.handle, op.handle, _pd(_f64(x)), _pd(_f64(b)), _pd(r)))
    return np.linalg.norm(r, 2)


def norm2(x, ctx=None):
    """||x||_2 of a DeviceVector (or of a host array, uploaded first) -- C ABI aggmg_norm2_dev"""
    c = ctx or getattr(x, "ctx", None) or default_context()
    dx = x if isinstance(x, DeviceVector) else c.to_device(_f64(x))
    out = ctypes.c_double(0.0)
    c.check(c.lib.aggmg_norm2_dev(c.handle, dx.ptr, dx.n, ctypes.byref(out)))
    return out.value


def dot(x, y, ctx=None):
    """x . y of two DeviceVectors (host arrays are uploaded first) -- C ABI aggmg_dot_dev"""
    c = ctx or getattr(x, "ctx", None) or default_context()
    dx = x if isinstance(x, DeviceVector) else c.to_device(_f64(x))
    dy = y if isinstance(y, DeviceVector) else c.to_device(_f64(y))
    if dx.n != dy.n:
        raise DimensionMismatch("dot: vectors differ in length")
    out = ctypes.c_double(0.0)
    c.check(c.lib.aggmg_dot_dev(c.handle, dx.ptr, dy.ptr, dx.n, ctypes.byref(out)))
    return out.value


class DirectSolver:
    """`A \\ b` for a device operator -- the fine-level direct solve behind the reference's `err` histories
    (`u_exact = H.mStiffness[1] \\ b`, src/solvers.jl:120; `uExact = A \\ b`, :194).  A one-level hierarchy of the operator
    IS the direct solve (src/solvers.jl:39): block cyclic reduction on the device when A is block-tridiagonal with
    well-conditioned pivot blocks (every DG / agglomerated operator; accepted on a probe solve, include/aggmg_hip.h);
    the same reduction in element-chain order when A is a CG operator of degree <= 8 (its vertices-first numbering has
    no band; in the order [left vertex, interior nodes] of every element it is block-tridiagonal with p x p blocks:
    COARSE_DEVICE_CHAIN, the chain form left by a chain smoother on the operator or detected in its pattern); the
    library's host banded LU otherwise; operators none of them takes are solved with SciPy's sparse LU on the host and
    the solution is uploaded -- once per call, not per cycle.
    `where` says which, tried in this order: 'device', 'device (element chain)', 'host banded LU', 'host sparse LU'."""

    def __init__(self, op, host_matrix=None):
        self.op, self.ctx = op, op.ctx
        self._host = host_matrix
        self.H = None
        self._lu = None
        # (each form once: the two device orders, then the host banded LU by name -- COARSE_AUTO would try both device
        # orders again before it gets there; on a CG operator the host factorisation is O(N^3))
        for mode in (_lib.COARSE_DEVICE_CR, _lib.COARSE_DEVICE_CHAIN, _lib.COARSE_HOST_BANDED):
            try:
                self.H = MeshHierarchy(None, [op], [], [], ctx=self.ctx, coarse_mode=mode)
                break
            except _lib.UnsupportedError:
                pass
        if self.H is None:
            self.where = "host sparse LU"
        else:
            info = self.H.coarse_info()
            self.where = ("host banded LU" if not info["on_device"] else
                          "device (element chain)" if info["order"] == "element chain" else "device")

    def solve_dev(self, b):
        """b: DeviceVector -> DeviceVector, or DeviceMatrix (N, K) -> DeviceMatrix (EXTENSION; Julia's `A \\ B` takes
        matrices): on the device the columns share every launch of the factorisation, a group at a time
        (MeshHierarchy.coarse_solve_multi_dev), and column j is bit for bit the solve of column j; the host sparse LU
        solves the downloaded matrix in one call"""
        N = self.op.shape[0]
        if isinstance(b, DeviceMatrix):
            if b.n != N:
                raise DimensionMismatch(f"DirectSolver.solve_dev: {b.n} rows, the operator has {N}")
            if self.H is not None:
                X = DeviceMatrix(self.ctx, N, b.k)
                self.H.coarse_solve_multi_dev(b, X)
                return X
            X = DeviceMatrix(self.ctx, N, b.k)
            X.upload(self._host_lu().solve(b.download()))
            return X
        if isinstance(b, np.ndarray):
            raise ArgumentError("DirectSolver.solve_dev: b must be a DeviceVector or a DeviceMatrix, not a host array")
        if self.H is not None:
            x, z = self.ctx.alloc(N), self.ctx.alloc(N)
            self.H.vcycle_dev(z, b, x, 0, 0, 1.0)
            return x
        return self.ctx.to_device(self._host_lu().solve(b.download()))

    def _host_lu(self):
        if self._lu is None:
            A = self._host if self._host is not None else self.op.to_scipy()
            self._lu = spla.splu(sp.csc_matrix(A))
        return self._lu


def _direct_solver(owner, op, host_matrix=None):
    """the DirectSolver of `op`, cached on `owner` (a hierarchy or a smoother: factored once, reused by every call)"""
    ds = owner.__dict__.get("_direct_solver")
    if ds is None or ds.op is not op:
        ds = DirectSolver(op, host_matrix)
        owner.__dict__["_direct_solver"] = ds
    return ds


def multigrid_dev(H, x0, b, maxiter, tol, check_every=1, nPre=3, nPost=3, alpha=2.0 / 3.0, u_exact=None):
    """The loop of multigrid (src/solvers.jl:122-134) resident on the device -- C ABI
    aggmg_multigrid_dev.  x0, b: DeviceVectors.  -> (x DeviceVector, cycles, res list) or, with u_exact (DeviceVector:
    the fine-level direct solution of :120), -> (x, cycles, res list, err list) with err[i] = ||x_i - u_exact||_2 (:128)
    formed on the device."""
    c = H.ctx
    N = H._ops[0].shape[0]
    if x0.n != N or b.n != N or (u_exact is not None and u_exact.n != N):
        raise DimensionMismatch("multigrid: x0 / b do not match the fine operator")
    x = c.alloc(N)
    nchk = max(1, -(-int(maxiter) // max(1, int(check_every))))
    hist, ehist = np.zeros(nchk), np.zeros(nchk)
    ncyc, nck = ctypes.c_int(0), ctypes.c_int(0)
    c.check(c.lib.aggmg_multigrid_dev(c.handle, H.handle, x0.ptr, b.ptr, int(maxiter), float(tol), int(check_every),
                                      int(nPre), int(nPost), float(alpha), x.ptr, _pd(hist),
                                      ctypes.byref(ncyc), ctypes.byref(nck), _ptr(u_exact),
                                      _pd(ehist) if u_exact is not None else None))
    if u_exact is None:
        return x, ncyc.value, hist[:nck.value].tolist()
    return x, ncyc.value, hist[:nck.value].tolist(), ehist[:nck.value].tolist()


def multigrid(H, x0, b, maxiter, tol, exact=True, check_every=1, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """multigrid(H, x0, b, maxiter, tol) -> (x, iter, res, err)  (src/solvers.jl:116-139).
    The whole loop runs on the device (aggmg_multigrid_dev): x0 and b go up once, x comes back once.  exact=True (the
    reference's contract, the default): `u_exact = H.mStiffness[1] \\ b` (:120) is solved once -- on the device where the
    fine operator is block-tridiagonal (DirectSolver) -- and err[i] = ||x_i - u_exact||_2 (:128) is formed on the device;
    exact=False skips the direct solve and returns err empty.  check_every = c > 1 runs c cycles per residual check in
    one fused device call; res / err then have one entry per check and `iter` counts cycles.  x0, b may be DeviceVectors,
    x then is one too.  nPre / nPost / alpha: multigrid_v_cycle's defaults, which the reference's loop uses (:125)."""
    if isinstance(b, DeviceMatrix) or (not isinstance(b, DeviceVector) and np.ndim(b) == 2):
        return _multigrid_multi(H, x0, b, maxiter, tol, exact, check_every, nPre, nPost, alpha)
    c = H.ctx
    on_device = isinstance(x0, DeviceVector) and isinstance(b, DeviceVector)
    dx0 = x0 if isinstance(x0, DeviceVector) else c.to_device(_f64(x0))
    db = b if isinstance(b, DeviceVector) else c.to_device(_f64(b))
    u_exact = None
    if exact:
        A0 = H.mStiffness[0]
        u_exact = _direct_solver(H, H._ops[0], None if isinstance(A0, DeviceOperator) else A0).solve_dev(db)
    out = multigrid_dev(H, dx0, db, maxiter, tol, check_every, nPre, nPost, alpha, u_exact)
    dx, ncyc, res = out[:3]
    err = out[3] if exact else []
    if int(maxiter) == 0:
        res, err = [], []
    return (dx if on_device else dx.download()), (ncyc if check_every > 1 else len(res)), res, err


def _copy_dev(c, dst, src, n):
    """n doubles from device address src to device address dst, on the context stream (C ABI aggmg_copy_segments_dev)"""
    if n <= 0:
        return
    one = lambda T, v: (T * 1)(v)
    c.check(c.lib.aggmg_copy_segments_dev(c.handle, 1, one(ctypes.c_void_p, src), one(ctypes.c_void_p, dst),
                                          one(ctypes.c_int64, 1), one(ctypes.c_int64, n), one(ctypes.c_int64, n),
                                          one(ctypes.c_int64, n)))


def _device_matrices(who, H, mats):
    """the (N, K) arguments of a K-column solver as DeviceMatrix objects: all DeviceMatrix (-> on_device True) or all host
    arrays in either memory order (uploaded); None entries stay None"""
    N = H._ops[0].shape[0]
    c = H.ctx
    given = [M_ for M_ in mats if M_ is not None]
    on_device = all(isinstance(M_, DeviceMatrix) for M_ in given)
    if not on_device and any(isinstance(M_, (DeviceMatrix, DeviceVector)) for M_ in given):
        raise ArgumentError(f"{who}: the matrices must be all DeviceMatrix or all host arrays")
    out = []
    shape = None
    for M_ in mats:
        if M_ is None:
            out.append(None)
            continue
        if not on_device:
            A_ = np.asarray(M_, dtype=np.float64)
            if A_.ndim != 2 or A_.shape[0] != N:
                raise DimensionMismatch(f"{who}: a matrix has shape {A_.shape}, expected ({N}, K)")
            if A_.shape[1] < 1:
                raise ArgumentError(f"{who}: a matrix has no columns")
            M_ = DeviceMatrix(c, N, A_.shape[1])
            M_.upload(A_)
        if M_.n != N or (shape is not None and M_.shape != shape):
            raise DimensionMismatch(f"{who}: the matrices do not match (N, K) of the fine operator")
        shape = M_.shape
        out.append(M_)
    return out, on_device


def _direct_solve_cols(H, dB):
    """U = H.mStiffness[1] \\ B through the hierarchy's DirectSolver, once: the columns in groups on the device"""
    A0 = H.mStiffness[0]
    ds = _direct_solver(H, H._ops[0], None if isinstance(A0, DeviceOperator) else A0)
    return ds.solve_dev(dB)


def _multigrid_multi(H, X0, B, maxiter, tol, exact, check_every, nPre, nPost, alpha):
    """multigrid on K right-hand sides (EXTENSION; the reference's takes vectors, src/solvers.jl:116-139): X0, B (N, K) host
    arrays or DeviceMatrix.  -> (X, cycles[K], res: K lists, err: K lists); column j's X, count and histories are those
    of multigrid on column j (C ABI aggmg_multigrid_multi_dev)."""
    (dX0, dB), on_device = _device_matrices("multigrid", H, [X0, B])
    if dX0 is None:
        raise ArgumentError("multigrid: X0 is needed (the reference's multigrid takes an initial guess)")
    U = _direct_solve_cols(H, dB) if exact else None
    dX = DeviceMatrix(H.ctx, dB.n, dB.k)
    ncyc, res, err, _ = H.multigrid_multi_dev(dX0, dB, dX, maxiter, tol, dB.k, dB.n, check_every, nPre, nPost, alpha, U)
    iters = ncyc if check_every > 1 else np.array([len(r) for r in res], dtype=np.int32)
    return (dX if on_device else dX.download()), iters, res, err


def _pcg_multi(H, B, X0, maxiter, tol, nPre, nPost, alpha):
    """pcg on K right-hand sides (EXTENSION): B, X0 (N, K) host arrays or DeviceMatrix, X0 None: zero guesses.
    -> (X, iters[K], res: K lists); column j is pcg on column j (C ABI aggmg_pcg_multi_dev).  X0 is not modified."""
    (dB, dX0), on_device = _device_matrices("pcg", H, [B, X0])
    c = H.ctx
    if dX0 is not None and not on_device:
        dX = dX0                             # (the uploaded copy of the caller's array)
    else:
        dX = DeviceMatrix(c, dB.n, dB.k)     # (aggmg_dev_alloc zeroes: the zero guesses)
        if dX0 is not None:
            _copy_dev(c, dX.ptr.value, dX0.ptr.value, dB.n * dB.k)
    its, res, _ = H.pcg_multi_dev(dB, dX, dB.k, dB.n, maxiter, tol, nPre, nPost, alpha)
    return (dX if on_device else dX.download()), its, res


def pcg(H, b, x0=None, maxiter=50, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """Conjugate gradients with ldiv!(y, H, r) (src/solvers.jl:84-92) as the preconditioner,
    resident on the device (C ABI aggmg_pcg_dev).  EXTENSION: the reference offers ldiv! for this
    use but has no Krylov loop.  -> (x, iter, res)
    Needs a symmetric positive definite operator AND a symmetric cycle (nPre == nPost, a sweep-weight schedule whose post
    half is the pre half reversed, no hybrid Schwarz level -- the multiplicative patch smoother, ElementPatchGaussSeidel,
    gives a symmetric cycle under the same two conditions); nothing checks that, and on another cycle the result is
    wrong without an error: use fgmres there."""
    if isinstance(b, DeviceMatrix) or (not isinstance(b, DeviceVector) and np.ndim(b) == 2):
        return _pcg_multi(H, b, x0, maxiter, tol, nPre, nPost, alpha)
    b = _f64(b)
    c = H.ctx
    N = H._ops[0].shape[0]
    if b.shape != (N,):
        raise DimensionMismatch("pcg: b does not match the fine operator")
    dx = c.to_device(np.zeros(N) if x0 is None else _f64(x0))
    db = c.to_device(b)
    hist = np.zeros(max(1, int(maxiter)))
    it = ctypes.c_int(0)
    c.check(c.lib.aggmg_pcg_dev(c.handle, H.handle, db.ptr, dx.ptr, int(maxiter), float(tol), int(nPre), int(nPost),
                                float(alpha), _pd(hist), ctypes.byref(it)))
    return dx.download(), it.value, hist[:it.value].tolist()


def fgmres(H, b, x0=None, restart=30, maxiter=200, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """Right-preconditioned flexible GMRES(restart) with one V-cycle from a zero guess as the preconditioner, resident on
    the device (C ABI aggmg_fgmres_dev).  EXTENSION: the reference has no Krylov loop.  Valid for EVERY cycle -- nPre !=
    nPost, unsymmetric sweep-weight schedules, hybrid Schwarz and Gauss-Seidel levels -- where pcg needs a symmetric one.
    -> (x, iter, res): res[i] the residual norm of the least-squares problem after iteration i; the loop stops when it is
    < tol ||b|| or after maxiter iterations.  b, x0 host arrays -> x a host array; DeviceVectors -> a DeviceVector.  x0
    (None: zeros) is not modified.  restart: iterations before the basis is dropped and the method starts again from the
    current residual, 1 .. 64; the work space is (2 restart + 2) vectors on the device.  Small values can stagnate where
    the default converges (restart 1 and 2 do on V(2,1) of the agglomerated DG hierarchy).  One
    right-hand side per call: fgmres_multi takes N x K matrices and runs the K recurrences in lockstep."""
    if isinstance(b, DeviceMatrix) or isinstance(x0, DeviceMatrix) or \
            (not isinstance(b, DeviceVector) and np.ndim(b) != 1):
        raise ArgumentError("fgmres: b must be one vector; K right-hand sides are out of scope of fgmres: use "
                            "fgmres_multi (pcg and multigrid take N x K matrices themselves)")
    c = H.ctx
    N = H._ops[0].shape[0]
    on_device = isinstance(b, DeviceVector)
    if x0 is not None and isinstance(x0, DeviceVector) != on_device:
        raise ArgumentError("fgmres: b and x0 must be both DeviceVectors or both host arrays")
    db = b if on_device else c.to_device(_f64(b))
    if db.n != N:
        raise DimensionMismatch("fgmres: b does not match the fine operator")
    if on_device:
        dx = DeviceVector(c, N)                 # (aggmg_dev_alloc zeroes: the zero guess)
        if x0 is not None:
            if x0.n != N:
                raise DimensionMismatch("fgmres: x0 does not match the fine operator")
            _copy_dev(c, dx.ptr.value, x0.ptr.value, N)
    else:
        x0 = np.zeros(N) if x0 is None else _f64(x0)
        if x0.shape != (N,):
            raise DimensionMismatch("fgmres: x0 does not match the fine operator")
        dx = c.to_device(x0)
    hist = np.zeros(max(1, int(maxiter)))
    it = ctypes.c_int(0)
    c.check(c.lib.aggmg_fgmres_dev(c.handle, H.handle, db.ptr, dx.ptr, int(restart), int(maxiter), float(tol), int(nPre),
                                   int(nPost), float(alpha), _pd(hist), ctypes.byref(it)))
    return (dx if on_device else dx.download()), it.value, hist[:it.value].tolist()


def fgmres_multi(H, B, X0=None, restart=30, maxiter=200, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """fgmres on K right-hand sides (EXTENSION): K recurrences in lockstep, one K-column cycle, one K-column operator
    product, one orthogonalisation launch sequence and one read-back per iteration (C ABI aggmg_fgmres_multi_dev; DESIGN.md
    24).  B, X0 (N, K) host arrays in either memory order, or DeviceMatrix; X0 None: zero guesses; X0 is not modified.
    -> (X, iters[K], res: K lists): column j's X, count and history are bit for bit those of fgmres on column j with the
    same arguments -- each column stops by its own ||b_j|| and then costs no further work.  Valid for every cycle, as
    fgmres.  The work space is (2 restart + 2) N x K matrices on the device."""
    (dB, dX0), on_device = _device_matrices("fgmres_multi", H, [B, X0])
    if dB is None:
        raise ArgumentError("fgmres_multi: B is needed")
    c = H.ctx
    if dX0 is not None and not on_device:
        dX = dX0                             # (the uploaded copy of the caller's array)
    else:
        dX = DeviceMatrix(c, dB.n, dB.k)     # (aggmg_dev_alloc zeroes: the zero guesses)
        if dX0 is not None:
            _copy_dev(c, dX.ptr.value, dX0.ptr.value, dB.n * dB.k)
    its, res, _ = H.fgmres_multi_dev(dB, dX, dB.k, dB.n, restart, maxiter, tol, nPre, nPost, alpha)
    return (dX if on_device else dX.download()), its, res


def iterative_smoother_solve(A, smoother, x0, b, maxiter=1000, tol=1e-6, alpha=1.0, exact=True, check_every=1):
    """iterative_smoother_solve(A, smoother, x0, b; maxiter=1000, tol=1e-6, alpha=1.0)
    -> (x, iter, res, err)  (src/solvers.jl:189-213).  Each iteration is one fused device sweep
    x = x0 + apply_smoother(S, b - A*x0; alpha); the loop, the residual norms and -- exact=True, the reference's contract
    and the default -- the error history err[i] = ||x_i - A \\ b||_2 (:194, :202) stay on the device
    (aggmg_smoother_solve_dev; the direct solve once, DirectSolver).  exact=False: err comes back empty."""
    op = smoother.A if not isinstance(A, DeviceOperator) else A
    c = op.ctx
    dx0, db = c.to_device(_f64(x0)), c.to_device(_f64(b))
    u_exact = None
    if exact:
        u_exact = _direct_solver(smoother, op, None if isinstance(A, DeviceOperator) else A).solve_dev(db)
    dx, nit, res, err = smoother_solve_dev(op, smoother, dx0, db, maxiter, tol, alpha, check_every=check_every, u_exact=u_exact)
    return dx.download(), (nit if check_every > 1 else len(res)), res, err


def smoother_solve_dev(A_op, smoother, x0, b, maxiter, tol, alpha=1.0, check_every=1, u_exact=None):
    """The loop of iterative_smoother_solve (src/solvers.jl:196-208) resident on the device -- C ABI
    aggmg_smoother_solve_dev.  x0, b (and u_exact, the direct solution of :194, or None): DeviceVectors.
    -> (x DeviceVector, iterations, res list, err list ([] without u_exact))."""
    c = A_op.ctx
    N = A_op.shape[0]
    if x0.n != N or b.n != N or (u_exact is not None and u_exact.n != N):
        raise DimensionMismatch("iterative_smoother_solve: x0 / b do not match the operator")
    dx = c.alloc(N)
    nchk = max(1, -(-int(maxiter) // max(1, int(check_every))))
    hist, ehist = np.zeros(nchk), np.zeros(nchk)
    nit, nck = ctypes.c_int(0), ctypes.c_int(0)
    c.check(c.lib.aggmg_smoother_solve_dev(c.handle, A_op.handle, smoother.handle, x0.ptr, b.ptr, int(maxiter),
                                           float(tol), float(alpha), int(check_every), dx.ptr, _pd(hist),
                                           ctypes.byref(nit), ctypes.byref(nck), _ptr(u_exact),
                                           _pd(ehist) if u_exact is not None else None))
    res = hist[:nck.value].tolist()
    err = ehist[:nck.value].tolist() if u_exact is not None else []
    return dx, nit.value, res, err


def chebyshev_weights(lam_max, degree=3, ratio=10.0, safety=1.05):
    """Sweep weights w_j = 1 / root_j of the degree-`degree` Chebyshev polynomial on [lo, hi] = [lam_max / ratio, safety *
    lam_max], smallest first (EXTENSION, no reference counterpart): `degree` sweeps u += w_j S^-1 (b - A u) multiply an
    error component of eigenvalue lam of S^-1 A by prod_j (1 - w_j lam), the polynomial with the smallest maximum over
    the interval, 1 / T_degree((hi + lo) / (hi - lo)).  lam_max: largest eigenvalue of S^-1 A
    (MeshHierarchy.estimate_lambda_max); safety covers an estimate from below."""
    lam_max, ratio, safety = float(lam_max), float(ratio), float(safety)
    if int(degree) != degree or degree < 1:
        raise ArgumentError("chebyshev_weights: degree must be a positive integer")
    if not (np.isfinite(lam_max) and lam_max > 0.0):
        raise ArgumentError("chebyshev_weights: lam_max must be positive and finite")
    if not (np.isfinite(ratio) and ratio > 1.0):
        raise ArgumentError("chebyshev_weights: ratio must be > 1")
    if not (np.isfinite(safety) and safety >= 1.0):
        raise ArgumentError("chebyshev_weights: safety must be >= 1")
    degree = int(degree)
    hi, lo = safety * lam_max, lam_max / ratio
    j = np.arange(degree)
    return 1.0 / (0.5 * (hi + lo) + 0.5 * (hi - lo) * np.cos(np.pi * (2 * j + 1) / (2 * degree)))


# stand-alone fused operations on host arrays (C ABI `aggmg_smooth`, `aggmg_residual`, ...)
def smooth(A_op, S, u, b, alpha=2.0 / 3.0, nsweeps=1):
    """nsweeps x `u += apply_smoother(S, b - A*u; alpha)` (src/solvers.jl:32-35) -> new vector.  EXTENSION: alpha may be
    a sequence -- sweep s is damped by alpha[s], nsweeps is then its length (C ABI aggmg_smooth_weighted_dev)."""
    u = _f64(u).copy()
    b = _f64(b)
    c = A_op.ctx
    if np.ndim(alpha) > 0:
        w = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).ravel())
        du, db = c.to_device(u), c.to_device(b)
        dout = c.alloc(u.size)
        try:
            c.check(c.lib.aggmg_smooth_weighted_dev(c.handle, A_op.handle, S.handle, du.ptr, db.ptr, _pd(w), w.size, dout.ptr))
            return dout.download()
        finally:
            for v in (du, db, dout):
                v.free()
    c.check(c.lib.aggmg_smooth(c.handle, A_op.handle, S.handle, _pd(u), _pd(b), float(alpha), int(nsweeps)))
    return u


def residual(A_op, u, b):
    """b - A*u (src/solvers.jl:33)"""
    r = np.empty(A_op.shape[0])
    c = A_op.ctx
    c.check(c.lib.aggmg_residual(c.handle, A_op.handle, _pd(_f64(u)), _pd(_f64(b)), _pd(r)))
    return r


def restrict(L_op, r):
    """L' * r (src/solvers.jl:36)"""
    rc = np.empty(L_op.shape[1])
    c = L_op.ctx
    c.check(c.lib.aggmg_restrict(c.handle, L_op.handle, _pd(_f64(r)), _pd(rc)))
    return rc


def prolong_add(L_op, uc, u):
    """u + L * uc (src/solvers.jl:42) -> new vector"""
    u = _f64(u).copy()
    c = L_op.ctx
    c.check(c.lib.aggmg_prolong_add(c.handle, L_op.handle, _pd(_f64(uc)), _pd(u)))
    return u


def smoother_launch_bytes(op, smoother=None, what="sweeps"):
    """(read, write) compulsory HBM bytes of one aggmg_smooth_dev launch (what='sweeps') or one aggmg_residual_dev
    launch (what='residual') on operator `op` (C ABI aggmg_smoother_launch_bytes): every array counted once."""
    ctx = op.ctx
    r, w = ctypes.c_int64(0), ctypes.c_int64(0)
    ctx.check(ctx.lib.aggmg_smoother_launch_bytes(ctx.handle, op.handle, smoother.handle if smoother is not None else None,
                                                  {"sweeps": 0, "residual": 1}[what], ctypes.byref(r), ctypes.byref(w)))
    return r.value, w.value
