"""Host-side mirror of the reference's operator interface for the hot path, over the C-ABI.

Same names, argument meaning and error behaviour as the classes `train-ctc-parallel` drives
(/root/reference/src/netbin/train-ctc-parallel.cc:111-119,195-207):

  Net  : Read, Write, SetTrainOptions, SetSeqLengths, InputDim, OutputDim, NumParams, GetParams, SetParams,
         Propagate, Backpropagate                      (/root/reference/src/net/net.h:48-161)
  Ctc  : EvalParallel, ErrorRateMSeq, Report, NumErrorTokens, NumRefTokens
                                                       (/root/reference/src/net/ctc-loss.h:40-63)
  Feeder : device-side minibatch assembly (train-ctc-parallel.cc:186-195), double-buffered
  CuMatrix : a [rows x cols] fp32 device matrix with a stride, the stand-in for CuMatrix<BaseFloat>
                                                       (/root/reference/src/gpucompute/cuda-matrix.h)

Errors surface as EesenError (the reference throws std::runtime_error from KALDI_ERR).  Everything here
is plumbing: all arithmetic happens in libeesen_hip.so.  No torch import — device memory comes from the
library's own allocator, so the product path has no framework dependency.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import EesenError, check


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class CuMatrix:
    """Row-major fp32 device matrix {rows, cols, stride} (/root/reference/src/gpucompute/cuda-matrixdim.h:52-56).

    Owns its memory when created with `CuMatrix(rows, cols)`; `CuMatrix.view(ptr, ...)` wraps memory owned
    by a Net (Propagate output).  Rows are padded to a multiple of 4 floats so they stay 16-byte aligned.
    """

    def __init__(self, rows: int, cols: int, device: int = 0, zero: bool = True):
        self.rows, self.cols, self.device = int(rows), int(cols), device
        self.stride = (self.cols + 3) & ~3
        self._own = True
        p = C.c_void_p()
        check(_lib.load().eesen_dev_alloc(device, max(1, self.rows * self.stride) * 4, C.byref(p)))
        self.ptr = p.value
        if zero and rows * cols:
            z = np.zeros(self.rows * self.stride, np.float32)
            check(_lib.load().eesen_dev_copy(device, C.c_void_p(self.ptr), _np_ptr(z), z.nbytes, 1))

    @classmethod
    def view(cls, ptr: int, rows: int, cols: int, stride: int, device: int = 0, keepalive=None) -> "CuMatrix":
        m = cls.__new__(cls)
        m.ptr, m.rows, m.cols, m.stride, m.device, m._own, m._keep = ptr, rows, cols, stride, device, False, keepalive
        return m

    @classmethod
    def from_numpy(cls, a: np.ndarray, device: int = 0) -> "CuMatrix":
        a = np.ascontiguousarray(a, np.float32)
        m = cls(a.shape[0], a.shape[1], device, zero=False)
        buf = np.zeros((m.rows, m.stride), np.float32)
        buf[:, : m.cols] = a
        check(_lib.load().eesen_dev_copy(device, C.c_void_p(m.ptr), _np_ptr(buf), buf.nbytes, 1))
        return m

    def NumRows(self) -> int:
        return self.rows

    def NumCols(self) -> int:
        return self.cols

    def Stride(self) -> int:
        return self.stride

    def numpy(self) -> np.ndarray:
        """CopyToMat: device -> host, dense [rows x cols]. Synchronous."""
        buf = np.empty((self.rows, self.stride), np.float32)
        if buf.size:
            check(_lib.load().eesen_dev_copy(self.device, _np_ptr(buf), C.c_void_p(self.ptr), buf.nbytes, 2))
        return np.ascontiguousarray(buf[:, : self.cols])

    def __del__(self):
        if getattr(self, "_own", False) and getattr(self, "ptr", None):
            try:
                _lib.load().eesen_dev_free(self.device, C.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = None


class Comm:
    """One rank of the data-parallel job: an RCCL communicator owned by libeesen_hip.so (include/eesen_hip.h
    `eesen_comm_*`), the replacement of the reference's file-based comm_avg_weights / comm_touch_done
    (/root/reference/src/net/communicator.h:39-170).  No torch involved: rank 0 hands the RCCL unique id to the other
    ranks over a plain TCP connection on MASTER_ADDR : (EESEN_COMM_PORT | MASTER_PORT + 17)."""

    SUM, MAX = 0, 1

    def __init__(self, device: int, rank: int, world: int, addr: str = "127.0.0.1", port: int = 29517, timeout_s: int = 120):
        self.lib = _lib.load()
        self.device, self.rank, self.world = device, rank, world
        self.h = C.c_void_p()
        check(self.lib.eesen_comm_create_tcp(device, addr.encode(), int(port), rank, world, int(timeout_s), C.byref(self.h)))

    @classmethod
    def from_env(cls, device: Optional[int] = None, timeout_s: int = 120) -> "Comm":
        """RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT as torch.distributed.run (or bench.py's own launcher) export them."""
        import os
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        dev = int(os.environ.get("LOCAL_RANK", "0")) if device is None else device
        port = int(os.environ.get("EESEN_COMM_PORT", 0)) or int(os.environ.get("MASTER_PORT", "29500")) + 17
        return cls(dev, rank, world, os.environ.get("MASTER_ADDR", "127.0.0.1"), port, timeout_s)

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_comm_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def allreduce(self, values: Sequence[float], op: int = 0) -> List[float]:
        """Sum (or max) of up to 64 host scalars over the ranks; blocks (also serves as a barrier)."""
        a = (C.c_double * len(values))(*[float(v) for v in values])
        check(self.lib.eesen_comm_allreduce_host(self.h, a, len(values), int(op)))
        return list(a)

    def barrier(self):
        self.allreduce([0.0])

    def Describe(self) -> dict:
        """COLLECTIVE (every rank calls it): the library the linker resolved, its version, whether it is the tests' stand-in, the
        ranks and device the library itself reports, every rank's PCI bus id, distinct_devices (eesen_comm_describe)."""
        import json
        buf = C.create_string_buffer(16384)
        check(self.lib.eesen_comm_describe(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())


class Net:
    """eesen::Net for BiLstmParallel / LstmParallel / AffineTransform / Softmax stacks."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = _lib.load()
        self.device = device
        self._stream = stream
        self.h = C.c_void_p()
        check(self.lib.eesen_net_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self._out = None
        self.grad_hook = None  # callable(net) run between backprop and update: the data-parallel exchange

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_net_destroy(self.h)
            except Exception:
                pass
            self.h = None

    # ---- model I/O ---------------------------------------------------------------------------
    def Read(self, path: str):
        """Net::Read (net.cc:279-309). Learn rate is reset to 0: call SetTrainOptions afterwards."""
        check(self.lib.eesen_net_read(self.h, path.encode()))
        return self

    def Write(self, path: str, binary: bool = True):
        check(self.lib.eesen_net_write(self.h, path.encode(), int(binary)))

    @classmethod
    def from_layers(cls, layers: List[dict], device: int = 0, stream: Optional[int] = None) -> "Net":
        """Build from the dict form of eesen_amd.nnet_io (type, input_dim, output_dim, learn_rate_coef, max_grad, params)."""
        net = cls(device, stream)
        for L in layers:
            check(net.lib.eesen_net_add_layer(net.h, _lib.KIND_OF[L["type"]], int(L["input_dim"]), int(L["output_dim"]),
                                              float(L.get("learn_rate_coef", 1.0)), float(L.get("max_grad", 0.0))))
        check(net.lib.eesen_net_finalize(net.h))
        flat = [np.asarray(p, np.float32).ravel() for L in layers for p in L["params"]]
        if flat:
            net.SetParams(np.concatenate(flat))
        for i, L in enumerate(layers):
            if L.get("dropout"):
                net.SetLayerDropout(i, L["dropout"])
        return net

    # ---- dropout (bilstm-parallel-layer.h:46-94) ------------------------------------------------
    def SetTrainMode(self):
        """Net::SetTrainMode (net.cc:405-412): dropout layers draw and apply their masks (the default)."""
        check(self.lib.eesen_net_set_train_mode(self.h, 1))

    def SetTestMode(self):
        """Net::SetTestMode (net.cc:396-403): no dropout."""
        check(self.lib.eesen_net_set_train_mode(self.h, 0))

    def SetLayerDropout(self, layer: int, opts: dict):
        """opts: keys of eesen_amd.nnet_io.DROPOUT_KEYS (forward, fw_step, fw_seq, rec_step, rec_seq, rnndrop, nml, recurrent, twiddle)."""
        from .nnet_io import dropout_values
        v = np.array([float(x) for x in dropout_values({"dropout": opts})], np.float32)
        check(self.lib.eesen_net_set_layer_dropout(self.h, layer, v.ctypes.data_as(C.POINTER(C.c_float))))

    def GetLayerDropout(self, layer: int) -> dict:
        from .nnet_io import DROPOUT_KEYS
        v = np.zeros(9, np.float32)
        check(self.lib.eesen_net_get_layer_dropout(self.h, layer, v.ctypes.data_as(C.POINTER(C.c_float))))
        return {k: (float(x) if k in ("forward", "recurrent") else bool(x)) for k, x in zip(DROPOUT_KEYS, v) if x}

    def SetDropoutSeed(self, seed: int):
        check(self.lib.eesen_net_set_dropout_seed(self.h, C.c_ulonglong(seed)))

    def SetDropoutMasks(self, layer: int, fwd=None, rec=None, twiddle_coin: int = -1):
        """Masks for the NEXT Propagate (parity tests): fwd [T*S x 2H]; rec [(T+2)*S x 2H] or [S x 2H] (fw columns, then bw)."""
        f = None if fwd is None else np.ascontiguousarray(fwd, np.float32)
        r = None if rec is None else np.ascontiguousarray(rec, np.float32)
        check(self.lib.eesen_net_set_dropout_masks(self.h, layer, _np_ptr(f) if f is not None else None, 0 if f is None else f.size,
                                                   _np_ptr(r) if r is not None else None, 0 if r is None else r.shape[0],
                                                   0 if r is None else r.size, int(twiddle_coin)))

    def GetDropoutMasks(self, layer: int, T: int, S: int) -> dict:
        """What the last Propagate applied to `layer`: dict(fwd [T*S x 2H] | None, rec [(T+2)*S x 2H] | None, mode, coin)."""
        info = (C.c_int * 4)()
        check(self.lib.eesen_net_get_dropout_masks(self.h, layer, None, None, info))
        w = info[3]
        fwd = np.zeros((T * S, w), np.float32) if info[0] else None
        rec = np.zeros(((T + 2) * S, w), np.float32) if info[1] else None
        check(self.lib.eesen_net_get_dropout_masks(self.h, layer, _np_ptr(fwd) if fwd is not None else None,
                                                   _np_ptr(rec) if rec is not None else None, info))
        return dict(fwd=fwd, rec=rec, mode=int(info[1]), coin=bool(info[2]))

    def layers(self) -> List[dict]:
        n = C.c_int()
        check(self.lib.eesen_net_num_layers(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            k, di, do, cf, mg = C.c_int(), C.c_int(), C.c_int(), C.c_float(), C.c_float()
            check(self.lib.eesen_net_layer_info(self.h, i, C.byref(k), C.byref(di), C.byref(do), C.byref(cf), C.byref(mg)))
            out.append(dict(type=_lib.NAME_OF[k.value], input_dim=di.value, output_dim=do.value,
                            learn_rate_coef=cf.value, max_grad=mg.value))
            dr = self.GetLayerDropout(i)
            if dr:
                out[-1]["dropout"] = dr
        return out

    def InputDim(self) -> int:
        d = C.c_int()
        check(self.lib.eesen_net_input_dim(self.h, C.byref(d)))
        return d.value

    def OutputDim(self) -> int:
        d = C.c_int()
        check(self.lib.eesen_net_output_dim(self.h, C.byref(d)))
        return d.value

    def NumParams(self) -> int:
        n = C.c_long()
        check(self.lib.eesen_net_num_params(self.h, C.byref(n)))
        return n.value

    def GetParams(self) -> np.ndarray:
        out = np.empty(self.NumParams(), np.float32)
        check(self.lib.eesen_net_get_params(self.h, _np_ptr(out), out.size))
        return out

    def SetParams(self, flat: np.ndarray):
        flat = np.ascontiguousarray(flat, np.float32)
        check(self.lib.eesen_net_set_params(self.h, _np_ptr(flat), flat.size))

    def GetGrads(self) -> np.ndarray:
        """Fresh gradients of the last Backpropagate in GetParams order (parity accessor)."""
        out = np.empty(self.NumParams(), np.float32)
        check(self.lib.eesen_net_get_grads(self.h, _np_ptr(out), out.size))
        return out

    # ---- options -----------------------------------------------------------------------------
    def SetTrainOptions(self, learn_rate: float, momentum: float = 0.0):
        check(self.lib.eesen_net_set_train_options(self.h, float(learn_rate), float(momentum)))

    def SetUpdateAlgorithm(self, name: str, adagrad_epsilon: float = 1e-6, rmsprop_rho: float = 0.9):
        """Net::SetUpdateAlgorithm (net.cc:481-497) + the adaptive hyper-parameters of NetTrainOptions."""
        check(self.lib.eesen_net_set_update_algorithm(self.h, name.encode()))
        check(self.lib.eesen_net_set_adaptive_options(self.h, float(adagrad_epsilon), float(rmsprop_rho)))

    def GetAccumulators(self) -> np.ndarray:
        out = np.empty(self.NumParams(), np.float32)
        check(self.lib.eesen_net_get_accumulators(self.h, _np_ptr(out), out.size))
        return out

    def SetAccumulators(self, flat: np.ndarray):
        flat = np.ascontiguousarray(flat, np.float32)
        check(self.lib.eesen_net_set_accumulators(self.h, _np_ptr(flat), flat.size))

    def SetSeqLengths(self, lens: Sequence[int]):
        a = np.ascontiguousarray(lens, np.int32)
        check(self.lib.eesen_net_set_seq_lengths(self.h, _np_ptr(a), a.size))

    # ---- compute -----------------------------------------------------------------------------
    def Propagate(self, feats) -> CuMatrix:
        """Net::Propagate (net.cc:67-86). feats: host ndarray [T*S x InputDim] (uploaded, as the reference's
        CuMatrix ctor does) or a CuMatrix.  Returns a view of the net-owned output, valid until the next call."""
        p, co, ld = C.c_void_p(), C.c_int(), C.c_int()
        if isinstance(feats, CuMatrix):
            check(self.lib.eesen_net_propagate(self.h, C.c_void_p(feats.ptr), feats.rows, feats.stride, 1, C.byref(p), C.byref(co), C.byref(ld)))
            rows = feats.rows
        else:
            a = np.ascontiguousarray(feats, np.float32)
            if a.ndim != 2:
                raise EesenError(-1, "Propagate expects a [rows x dim] matrix")
            check(self.lib.eesen_net_propagate(self.h, _np_ptr(a), a.shape[0], a.shape[1], 0, C.byref(p), C.byref(co), C.byref(ld)))
            rows = a.shape[0]
        self._out = CuMatrix.view(p.value, rows, co.value, ld.value, self.device, keepalive=self)
        return self._out

    def BackpropagateNoUpdate(self, out_diff: CuMatrix, in_diff: Optional[CuMatrix] = None):
        check(self.lib.eesen_net_backpropagate(self.h, C.c_void_p(out_diff.ptr), out_diff.stride,
                                               C.c_void_p(in_diff.ptr) if in_diff is not None else None,
                                               in_diff.stride if in_diff is not None else 0))

    def Update(self):
        check(self.lib.eesen_net_update(self.h))

    def Backpropagate(self, out_diff: CuMatrix, in_diff: Optional[CuMatrix] = None):
        """Net::Backpropagate (net.cc:88-108): gradients, [data-parallel exchange], per-layer Update."""
        self.BackpropagateNoUpdate(out_diff, in_diff)
        if self.grad_hook is not None:
            self.grad_hook(self)
        self.Update()

    def SetComm(self, comm: Optional[Comm]):
        """Attach the data-parallel communicator: Backpropagate then all-reduces every layer's fresh gradients (one bucket per
        layer, on the communicator's stream, under the lower layers' backward pass) and Update waits bucket by bucket."""
        check(self.lib.eesen_net_set_comm(self.h, comm.h if comm is not None else None))
        self._comm = comm

    def AllReduceGrads(self, comm: Comm):
        """The bulk form: one all-reduce of the whole gradient buffer, between BackpropagateNoUpdate and Update."""
        check(self.lib.eesen_net_allreduce_grads(self.h, comm.h))

    def BackpropagateZero(self):
        """This rank has no minibatch this step (others do): zero gradient through the same collectives; then Update()."""
        check(self.lib.eesen_net_backpropagate_zero(self.h))

    def LiveRanks(self) -> int:
        """How many ranks had a minibatch in the step issued last (the liveness word that rides with the top layer's gradient
        bucket).  For a rank in the zero-gradient protocol: 0 = every rank is out of data.  Blocks until that bucket has arrived."""
        n = C.c_int()
        check(self.lib.eesen_net_live_ranks(self.h, C.byref(n)))
        return n.value

    def LayerMarker(self, idx: int) -> str:
        buf = C.create_string_buffer(64)
        check(self.lib.eesen_net_layer_marker(self.h, idx, buf, 64))
        return buf.value.decode()

    def TensorMoments(self, which: int, layer: int) -> np.ndarray:
        """[n_tensors x 6] = (min, max, mean, variance, skewness, kurtosis) per tensor of `layer`, in the order of the reference
        layer's Info(); which: 0 parameters, 1 momentum buffers (*_corr_), 2 adaptive accumulators."""
        n = C.c_int()
        check(self.lib.eesen_net_tensor_moments(self.h, which, layer, None, 0, C.byref(n)))
        out = np.zeros((n.value, 6), np.float64)
        if n.value:
            check(self.lib.eesen_net_tensor_moments(self.h, which, layer, out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return out

    def Info(self) -> str:
        """Net::Info (net.cc:336-354): topology + MomentStatistics of every parameter tensor."""
        return _net_info(self, 0)

    def InfoGradient(self, with_accumulators: bool = False) -> str:
        """Net::InfoGradient (net.cc:356-366): MomentStatistics of every momentum buffer (*_corr_); with_accumulators: followed by
        those of the adaptive accumulators, as the reference's layers print them once an adaptive rule has run
        (bilstm-layer.h:515-531, affine-trans-layer.h:150-155)."""
        return _net_info(self, 1, with_accumulators)

    def BucketOrder(self) -> List[int]:
        buf = (C.c_int * 64)()
        n = C.c_int()
        check(self.lib.eesen_net_bucket_order(self.h, buf, 64, C.byref(n)))
        return list(buf[: n.value])

    def grad_buffer(self):
        """(device pointer, float count) of the contiguous fresh-gradient buffer (all-reduce payload)."""
        p, n = C.c_void_p(), C.c_long()
        check(self.lib.eesen_net_grad_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def SetForwardPrecision(self, bf16):
        """BASELINE config 4's bf16 forward (eesen_net_set_forward_precision): True / 1 = forward GEMMs AND the forward time
        recurrence on bf16 operands with fp32 accumulation; 2 = the GEMMs only; False / 0 = fp32.  Everything else stays fp32."""
        check(self.lib.eesen_net_set_forward_precision(self.h, int(bf16)))

    def Bf16RecurrenceLayers(self) -> int:
        """LSTM layers of the last Propagate whose recurrence ran on the bf16 kernel (debug accessor)."""
        n = C.c_int()
        check(self.lib.eesen_net_bf16_recurrence_layers(self.h, C.byref(n)))
        return n.value

    def RecurrenceInfo(self) -> dict:
        """Which recurrence kernels the last Propagate / Backpropagate used (debug accessor)."""
        a = (C.c_int * 4)()
        check(self.lib.eesen_net_recurrence_info(self.h, a))
        self.recoveries = a[3]
        return dict(lstm_layers=a[0], fwd_persistent=a[1], bwd_persistent=a[2])

    def Plan(self) -> dict:
        """What will run the current minibatch shape (after SetSeqLengths): the recurrence plans of every LSTM layer -- the very ones
        the launchers execute -- and the schedule decisions read from them (eesen_net_plan_string)."""
        import json
        buf = C.create_string_buffer(32768)
        check(self.lib.eesen_net_plan_string(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def _raise_error_word(self, value: int):
        """Test hook: what a recurrence kernel (1) / the milestone waiter (2) stores when it gives up."""
        check(self.lib.eesen_net_debug_set_error_word(self.h, int(value)))

    def DebugLayerBuffer(self, layer: int, which: int) -> np.ndarray:
        """Test hook (eesen_net_debug_layer_buffer): the T*S interior rows of LSTM layer `layer`'s gate activations (0), cell state
        c (1), unmasked output m (2) or gate gradients DG (3), in the model file's column order (per direction g, i, f, o)."""
        r, c = C.c_int(0), C.c_int(0)
        check(self.lib.eesen_net_debug_layer_buffer(self.h, int(layer), int(which), None, 0, C.byref(r), C.byref(c)))
        buf = np.empty((r.value, c.value), np.float32)
        check(self.lib.eesen_net_debug_layer_buffer(self.h, int(layer), int(which), _np_ptr(buf), buf.size, C.byref(r), C.byref(c)))
        return buf

    def Synchronize(self):
        check(self.lib.eesen_net_synchronize(self.h))

    def SetProfiling(self, on, accumulate: bool = False):
        """HIP-event phase timers: per step (read after every step), or accumulated over several steps until PhaseTimes()."""
        check(self.lib.eesen_net_set_profiling(self.h, 2 if (on and accumulate) else int(bool(on))))

    def PhaseSpans(self):
        """[(phase name, seconds)] of every timed span since the last PhaseTimes(), in record order (call before PhaseTimes)."""
        names = ["input_gemm", "recurrence_fwd", "affine_softmax", "recurrence_bwd", "grad_gemm", "update", "allreduce", "allreduce_exposed"]
        n = C.c_int()
        check(self.lib.eesen_net_get_phase_spans(self.h, None, None, 0, C.byref(n)))
        ph, se = (C.c_int * max(n.value, 1))(), (C.c_float * max(n.value, 1))()
        check(self.lib.eesen_net_get_phase_spans(self.h, ph, se, n.value, C.byref(n)))
        return [(names[ph[i]] if 0 <= ph[i] < len(names) else str(ph[i]), float(se[i])) for i in range(n.value)]

    def PhaseTimes(self) -> dict:
        out = np.zeros(6, np.float32)
        check(self.lib.eesen_net_get_phase_times(self.h, _np_ptr(out)))
        return dict(zip(["input_gemm", "recurrence_fwd", "affine_softmax", "recurrence_bwd", "grad_gemm", "update"], out.tolist()))


_LSTM_TENSORS = ["wei_gifo_x", "wei_gifo_m", "bias", "phole_i_c", "phole_f_c", "phole_o_c"]


def _g(v: float) -> str:
    """What operator<< prints for a float by default (6 significant digits, printf's %g) -- a NaN with its sign: 0 / 0 of a constant
    tensor's skewness reads `-nan` or `nan` by the sign bit there, and include/eesen_hip_info.h prints the same doubles that way."""
    if v != v:
        import math
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return f"{v:g}"


def _net_info(net: "Net", which: int, with_accumulators: bool = False) -> str:
    """The strings of Net::Info / Net::InfoGradient (net.cc:336-366) with the per-layer parts of bilstm-layer.h:496-560,
    lstm-layer.h:175-196, affine-trans-layer.h:145-159; the same text as include/eesen_hip_info.h::NetInfo."""
    layers = net.layers()
    out = []
    if which == 0:
        out += [f"num-layers {len(layers)}", f"input-dim {net.InputDim()}", f"output-dim {net.OutputDim()}",
                f"number-of-parameters {_g(net.NumParams() / 1e6)} millions"]
    else:
        out.append("### Gradient stats :")
    for i, L in enumerate(layers):
        fmt = lambda m: [f" ( min {_g(r[0])}, max {_g(r[1])}, mean {_g(r[2])}, variance {_g(r[3])}, skewness {_g(r[4])}, kurtosis {_g(r[5])} ) "
                         for r in m]
        stats = fmt(net.TensorMoments(which, i))
        accu = fmt(net.TensorMoments(2, i)) if which == 1 and with_accumulators else []
        suf = "" if which == 0 else "corr_"
        body = ""
        if L["type"] in ("BiLstmParallel", "LstmParallel"):
            dirs = ["_fw_", "_bw_"] if L["type"] == "BiLstmParallel" else ["_"]
            names = [f"{t}{d}{suf}" for d in dirs for t in _LSTM_TENSORS]
            body = "    " + "".join(f"\n  {nm}  {st}" for nm, st in zip(names, stats))
            if L["type"] == "BiLstmParallel":     # (lstm-layer.h prints no accumulators)
                body += "".join(f"\n  {nm}accu  {st}" for nm, st in zip(names, accu))
        elif L["type"] == "AffineTransform":
            names = ["linearity", "bias"] if which == 0 else ["linearity_corr_", "bias_corr_"]
            body = "".join(f"\n  {nm}{st}" for nm, st in zip(names, stats))
            body += "".join(f"\n  {nm}{st}" for nm, st in zip(["linearity_grad_accu", "bias_grad_accu"], accu))
        marker = net.LayerMarker(i)
        if which == 0:
            out.append(f"layer {i + 1} : {marker}, input-dim {L['input_dim']}, output-dim {L['output_dim']}, {body}")
        else:
            out.append(f"Layer {i + 1} : {marker}, {body}")
    return "\n".join(out) + "\n"


class TokenLm:
    """A token n-gram LM for Ctc.DecodeParallel(lm=...): an ARPA file over the net's own tokens compiled into a deterministic backoff
    automaton (eesen_lm_create_from_arpa; INTEGRATION.md "LM fusion").  units: the recipes' units.txt (`symbol id` per line); without
    it the ARPA's words are decimal class ids.  K: the net's class count, blank included.  Host only: needs no device."""

    def __init__(self, arpa: str, units: Optional[str] = None, K: int = 0, skip_oov: bool = False):
        """skip_oov: n-grams with a word outside the table are dropped and counted (OovDropped) instead of being an error
        (eesen_lm_create_from_arpa_ex) -- what a word LM over a lexicon's words table usually needs."""
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.K = int(K)
        if skip_oov:
            check(self.lib.eesen_lm_create_from_arpa_ex(str(arpa).encode(), str(units).encode() if units else None, int(K), 1, C.byref(self.h)))
        else:
            check(self.lib.eesen_lm_create_from_arpa(str(arpa).encode(), str(units).encode() if units else None, int(K), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_lm_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def OovDropped(self) -> int:
        n = C.c_longlong()
        check(self.lib.eesen_lm_oov_dropped(self.h, C.byref(n)))
        return n.value

    def Info(self) -> dict:
        o, st, ar, eos = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.lib.eesen_lm_info(self.h, C.byref(o), C.byref(st), C.byref(ar), C.byref(eos)))
        return dict(order=o.value, states=st.value, arcs=ar.value, has_eos=bool(eos.value))

    def Start(self) -> int:
        st = C.c_int()
        check(self.lib.eesen_lm_start(self.h, C.byref(st)))
        return st.value

    def Step(self, state: int, c: int) -> Tuple[float, int]:
        """lm_step: (ln P(c | state) as the fp32 sum the device forms, the next state)."""
        w, nx = C.c_float(), C.c_int()
        check(self.lib.eesen_lm_step(self.h, int(state), int(c), C.byref(w), C.byref(nx)))
        return w.value, nx.value

    def Final(self, state: int) -> float:
        w = C.c_float()
        check(self.lib.eesen_lm_final(self.h, int(state), C.byref(w)))
        return w.value

    def Score(self, labels: Sequence[int], eos: bool = False, with_abs: bool = False):
        """ln P_lm(labels [, </s>]) in fp64 on the stored fp32 weights; with_abs: (that, the sum of the weights' magnitudes)."""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        v, a = C.c_double(), C.c_double()
        check(self.lib.eesen_lm_score(self.h, _np_ptr(lab) if lab.size else None, int(lab.size), int(bool(eos)), C.byref(v), C.byref(a)))
        return (v.value, a.value) if with_abs else v.value


class Lexicon:
    """A lexicon for Ctc.DecodeParallel(lexicon=...): `word unit unit ...` lines compiled into a trie (eesen_lex_create; INTEGRATION.md
    "Lexicon").  units: the recipes' units.txt; without it the units are decimal class ids (lexicon_numbers.txt).  K: the net's class
    count, blank included; space: the class that separates words.  space=None: the unspaced kind (eesen_lex_create_unspaced;
    INTEGRATION.md "Words without a boundary unit"): no boundary unit, several words per spelling; Ctc.DecodeParallel then takes
    eesen_ctc_decode_parallel_words.  Host only: needs no device."""

    def __init__(self, path: str, units: Optional[str] = None, K: int = 0, space: Optional[int] = 0):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.K, self.space, self.unspaced = int(K), space if space is None else int(space), space is None
        enc = str(units).encode() if units else None
        if self.unspaced:
            check(self.lib.eesen_lex_create_unspaced(str(path).encode(), enc, int(K), C.byref(self.h)))
        else:
            check(self.lib.eesen_lex_create(str(path).encode(), enc, int(K), int(space), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_lex_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def Info(self) -> dict:
        w, n, m = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.eesen_lex_info(self.h, C.byref(w), C.byref(n), C.byref(m)))
        return dict(words=w.value, nodes=n.value, max_word_len=m.value)

    def WriteWords(self, path: str) -> None:
        """`word id` lines: the units table of a word LM, TokenLm(arpa, path, K=words + 1)."""
        check(self.lib.eesen_lex_write_words(self.h, str(path).encode()))

    def Child(self, node: int, c: int) -> int:
        """The child of a trie node for class c, or -1."""
        ch = C.c_int()
        check(self.lib.eesen_lex_child(self.h, int(node), int(c), C.byref(ch)))
        return ch.value

    def Word(self, node: int) -> int:
        """The id (1 .. words) of the word whose spelling ends at the node, or 0."""
        w = C.c_int()
        check(self.lib.eesen_lex_word(self.h, int(node), C.byref(w)))
        return w.value

    def MaxHomophones(self) -> int:
        """H: the largest number of words on one spelling (0 for a lexicon with a space class)."""
        h = C.c_int()
        check(self.lib.eesen_lex_max_homophones(self.h, C.byref(h)))
        return h.value

    def NodeWords(self, node: int) -> List[int]:
        """The ascending ids of the words whose spelling ends at the node."""
        out = np.empty(16, np.int32)
        n = C.c_int()
        check(self.lib.eesen_lex_node_words(self.h, int(node), _np_ptr(out), int(out.size), C.byref(n)))
        return out[:n.value].tolist()

    def Lookahead(self, lm: "TokenLm") -> np.ndarray:
        """The unigram look-ahead table of a word LM over this lexicon (eesen_lex_lookahead; INTEGRATION.md "LM look-ahead"):
        float32 [nodes], la[v] = the largest unigram weight among the words whose spelling passes through or ends at node v."""
        out = np.empty(self.Info()["nodes"], np.float32)
        check(self.lib.eesen_lex_lookahead(self.h, lm.h, _np_ptr(out), int(out.size)))
        return out

    def Words(self, labels: Sequence[int]) -> List[int]:
        """The word ids of a labelling `w1 space w2 ... wn`; EesenError for a labelling that is none, and for an unspaced lexicon."""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        out = np.empty(lab.size // 2 + 1, np.int32)
        n = C.c_int()
        check(self.lib.eesen_lex_words(self.h, _np_ptr(lab) if lab.size else None, int(lab.size), _np_ptr(out), C.byref(n)))
        return out[:n.value].tolist()


class Stamps:
    """What Ctc.DecodeStamps returns: frame intervals [start, end) per label and per word, word confidences, best-path scores."""

    def __init__(self, label_start, label_end, word_start, word_end, word_conf, path_score):
        self.label_start, self.label_end = label_start, label_end
        self.word_start, self.word_end, self.word_conf = word_start, word_end, word_conf
        self.path_score = path_score


class Rescored:
    """What Ctc.RescoreNbest returns: exact acoustic scores, LM scores and totals [S, nbest], and the new order of the first-pass ranks."""

    def __init__(self, am_score, lm_score, total, order):
        self.am_score, self.lm_score, self.total, self.order = am_score, lm_score, total, order


class Mbr:
    """What Ctc.MbrNbest returns: dist [S, nbest, nbest] and ref_dist [S, nbest] int32 (-1 where an entry does not count; ref_dist is
    None without refs), posterior and risk [S, nbest] float64 (-1e30 there), order [S, nbest] int32 -- the first-pass ranks by risk."""

    def __init__(self, dist, ref_dist, posterior, risk, order):
        self.dist, self.ref_dist, self.posterior, self.risk, self.order = dist, ref_dist, posterior, risk, order


def word_confidence(scores, word_len, word_ids, wstart, wend, conf_scale: float = 1.0) -> np.ndarray:
    """N-best posterior word confidences on the host in fp64 (eesen_word_confidence; no device work).  scores [n]; word_len [n] (< 0:
    not an entry); word_ids / wstart / wend [n, stride].  Returns conf [n, stride] float64, -1e30 beyond each entry's words."""
    z = np.ascontiguousarray(scores, np.float64)
    wl = np.ascontiguousarray(word_len, np.int32)
    ids, b, e = (np.ascontiguousarray(a, np.int32).reshape(z.size, -1) for a in (word_ids, wstart, wend))
    if not (wl.size == z.size and ids.shape == b.shape == e.shape):
        raise EesenError(-1, "word_confidence: array shapes differ")
    out = np.empty(ids.shape, np.float64)
    check(_lib.load().eesen_word_confidence(z.size, _np_ptr(z), _np_ptr(wl), _np_ptr(ids), _np_ptr(b), _np_ptr(e), ids.shape[1],
                                            float(conf_scale), _np_ptr(out)))
    return out


class Ctc:
    """eesen::Ctc (ctc-loss.h:31-90) for the multi-sequence path."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = _lib.load()
        self.device = device
        self.h = C.c_void_p()
        check(self.lib.eesen_ctc_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.pzx = None

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_ctc_destroy(self.h)
            except Exception:
                pass
            self.h = None

    @staticmethod
    def _csr(label: Sequence[Sequence[int]]):
        off = np.zeros(len(label) + 1, np.int32)
        off[1:] = np.cumsum([len(l) for l in label])
        ids = np.concatenate([np.asarray(l, np.int32) for l in label]) if off[-1] else np.zeros(1, np.int32)
        return np.ascontiguousarray(ids, np.int32), off

    def EvalParallel(self, frame_num_utt: Sequence[int], net_out: CuMatrix, label: Sequence[Sequence[int]],
                     diff: Optional[CuMatrix] = None, want_pzx: bool = True) -> CuMatrix:
        """Ctc::EvalParallel (ctc-loss.cc:101-194). Returns diff (allocated when not given); self.pzx = ln p per sequence.
        want_pzx=False: nothing waits for the device -- ln p joins the objective sum (stats()) when it has arrived, as the
        reference's own call returns nothing but `diff` and only accumulates obj_progress_ (:171-177); self.pzx is None then."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        ids, off = self._csr(label)
        if diff is None:
            diff = CuMatrix(net_out.rows, net_out.cols, self.device, zero=False)
        pzx = np.empty(fn.size, np.float32) if want_pzx else None
        check(self.lib.eesen_ctc_eval_parallel(self.h, _np_ptr(fn), fn.size, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                               net_out.stride, _np_ptr(ids), _np_ptr(off), C.c_void_p(diff.ptr), diff.stride,
                                               _np_ptr(pzx) if want_pzx else None))
        self.pzx = pzx
        return diff

    def AlignParallel(self, frame_num_utt: Sequence[int], net_out: CuMatrix, label: Sequence[Sequence[int]], is_log: bool = False):
        """Best-path (Viterbi) CTC alignment (eesen_ctc_align_parallel; no counterpart in the reference's src/net).  net_out: posteriors,
        or log-domain scores with is_log=True.  Returns (ali [T, S] int32 class id per frame, pos [T, S] int32 lattice position,
        score [S] float32).  Ties: the smallest move wins (stay, j-1, j-2), the final blank wins over the last label.  Rows past an
        utterance's length are -1; an utterance without a feasible path has score -1e30 and -1 everywhere.  Statistics untouched."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        ids, off = self._csr(label)
        S = fn.size
        ali = np.empty(net_out.rows, np.int32)
        pos = np.empty(net_out.rows, np.int32)
        score = np.empty(S, np.float32)
        check(self.lib.eesen_ctc_align_parallel(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols, net_out.stride,
                                                int(bool(is_log)), _np_ptr(ids), _np_ptr(off), _np_ptr(ali), _np_ptr(pos), _np_ptr(score)))
        return ali.reshape(-1, S), pos.reshape(-1, S), score

    def AlignTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_align_times(self.h, _np_ptr(out)))
        return dict(zip(["log", "sweep", "traceback"], out.tolist()))

    def DecodeParallel(self, frame_num_utt: Sequence[int], net_out: CuMatrix, beam: int = 16, max_classes: int = 20, nbest: int = 1,
                       is_log: bool = False, lm: Optional["TokenLm"] = None, lm_weight: float = 1.0, insertion_bonus: float = 0.0,
                       lm_eos: bool = False, lexicon: Optional["Lexicon"] = None, word_bonus: float = 0.0,
                       lm_lookahead: Optional[bool] = None):
        """CTC prefix beam search (eesen_ctc_decode_parallel; no counterpart in the reference's src/net).  net_out: posteriors,
        or log-domain scores with is_log=True.  Returns (hyps, scores): hyps[s] is the list of the utterance's returned labellings, best
        first, each a list of ints (at most nbest; none where the beam died); scores [S, nbest] float32, -1e30 beyond the returned
        count (NaN under a raised guard word).  Statistics untouched.
        lm: a TokenLm fused into the search (eesen_ctc_decode_parallel_lm): every label adds lm_weight * ln P_lm(label | prefix) +
        insertion_bonus, with lm_eos lm_weight * ln P_lm(</s> | labels) joins at the end; self.lm_score [S, nbest] is then each
        entry's unweighted ln P_lm (None without an LM).  lm=None is the plain call.
        lexicon: a Lexicon the labellings are held to (eesen_ctc_decode_parallel_lex): words of the lexicon separated by single
        spaces.  lm is then an LM over the lexicon's word ids (TokenLm over Lexicon.WriteWords' table, K = words + 1) or None, stepped
        once per word; word_bonus is added per word and insertion_bonus is not used.  self.words [S, nbest, T] / self.words_len
        [S, nbest] are the word ids of every returned labelling (-1 beyond; None without a lexicon).  lexicon=None takes the calls
        above unchanged.  An unspaced lexicon (Lexicon(space=None)) takes eesen_ctc_decode_parallel_words: a returned entry is a
        labelling and a segmentation of it into words, homophones and other segmentations of the same labels are entries of their
        own, and self.word_ends [S, nbest, T] is the number of labels up to and including each word's last (-1 beyond the word
        count; None in every other mode).
        lm_lookahead: True / False sets the unigram LM look-ahead (SetLmLookahead; INTEGRATION.md "LM look-ahead") for this call and
        restores the object's mode behind it; None (the default) decodes in the object's mode.  True needs a lexicon and an lm."""
        if lm_lookahead is not None:
            if lm_lookahead and lexicon is None:
                raise EesenError(-1, "the LM look-ahead needs a lexicon and the word LM over it: this call has no lexicon")
            before = self.LmLookahead()
            self.SetLmLookahead(1 if lm_lookahead else 0)
            try:
                return self.DecodeParallel(frame_num_utt, net_out, beam, max_classes, nbest, is_log, lm, lm_weight, insertion_bonus, lm_eos,
                                           lexicon, word_bonus)
            finally:
                self.SetLmLookahead(before)
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        S = fn.size
        T = net_out.rows // max(S, 1)
        hyp = np.empty((S, int(nbest), max(T, 0)), np.int32)
        hlen = np.empty((S, int(nbest)), np.int32)
        score = np.empty((S, int(nbest)), np.float32)
        words = words_len = word_ends = None
        if lexicon is not None and lexicon.unspaced:
            lm_score = np.empty((S, int(nbest)), np.float32)
            words = np.empty((S, int(nbest), max(T, 0)), np.int32)
            word_ends = np.empty((S, int(nbest), max(T, 0)), np.int32)
            words_len = np.empty((S, int(nbest)), np.int32)
            check(self.lib.eesen_ctc_decode_parallel_words(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                                           net_out.stride, int(bool(is_log)), int(beam), int(max_classes), int(nbest), lexicon.h,
                                                           lm.h if lm is not None else None, float(lm_weight), float(word_bonus),
                                                           int(bool(lm_eos)), _np_ptr(hyp), _np_ptr(hlen), _np_ptr(score), _np_ptr(lm_score),
                                                           _np_ptr(words), _np_ptr(words_len), _np_ptr(word_ends)))
        elif lexicon is not None:
            lm_score = np.empty((S, int(nbest)), np.float32)
            words = np.empty((S, int(nbest), max(T, 0)), np.int32)
            words_len = np.empty((S, int(nbest)), np.int32)
            check(self.lib.eesen_ctc_decode_parallel_lex(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                                         net_out.stride, int(bool(is_log)), int(beam), int(max_classes), int(nbest), lexicon.h,
                                                         lm.h if lm is not None else None, float(lm_weight), float(word_bonus),
                                                         int(bool(lm_eos)), _np_ptr(hyp), _np_ptr(hlen), _np_ptr(score), _np_ptr(lm_score),
                                                         _np_ptr(words), _np_ptr(words_len)))
        elif lm is None:
            lm_score = None
            check(self.lib.eesen_ctc_decode_parallel(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols, net_out.stride,
                                                     int(bool(is_log)), int(beam), int(max_classes), int(nbest), _np_ptr(hyp), _np_ptr(hlen),
                                                     _np_ptr(score)))
        else:
            lm_score = np.empty((S, int(nbest)), np.float32)
            check(self.lib.eesen_ctc_decode_parallel_lm(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                                        net_out.stride, int(bool(is_log)), int(beam), int(max_classes), int(nbest), lm.h,
                                                        float(lm_weight), float(insertion_bonus), int(bool(lm_eos)), _np_ptr(hyp),
                                                        _np_ptr(hlen), _np_ptr(score), _np_ptr(lm_score)))
        self.hyp, self.hyp_len = hyp, hlen          # the raw [S, nbest, T] labels (-1 beyond each length) and [S, nbest] lengths
        self.lm_score = lm_score
        self.words, self.words_len, self.word_ends = words, words_len, word_ends
        hyps = [[hyp[s, i, :hlen[s, i]].tolist() for i in range(int(nbest)) if hlen[s, i] >= 0] for s in range(S)]
        return hyps, score

    def DecodeTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_decode_times(self.h, _np_ptr(out)))
        return dict(zip(["topc", "beam", "hyp"], out.tolist()))

    def DecodeStamps(self, frame_num_utt: Sequence[int], net_out: CuMatrix, is_log: bool = False, conf_scale: float = 1.0) -> "Stamps":
        """Time stamps and confidences of the entries the last DecodeParallel returned (eesen_ctc_decode_stamps; INTEGRATION.md "Time
        stamps and CTM").  frame_num_utt, net_out, is_log: that call's.  Every entry is aligned on the acoustic scores by AlignParallel's
        recurrence and tie rule, all of them in one launch.  Returns a Stamps: label_start / label_end / word_start / word_end
        [S, nbest, T] int32 (frames, end exclusive, -1 beyond the labels / words), word_conf [S, nbest, T] float32 (N-best posterior
        of the word, -1e30 beyond the words), path_score [S, nbest] float32.  The words are those of self.hyp / self.words /
        self.word_ends."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        S = fn.size
        hlen = getattr(self, "hyp_len", None)
        nbest = hlen.shape[1] if hlen is not None and hlen.shape[0] == S else 1   # (without a decode call the library refuses)
        T = net_out.rows // max(S, 1)
        shape = (S, nbest, max(T, 0))
        ls, le, ws, we = (np.empty(shape, np.int32) for _ in range(4))
        wc = np.empty(shape, np.float32)
        ps = np.empty((S, nbest), np.float32)
        check(self.lib.eesen_ctc_decode_stamps(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols, net_out.stride,
                                               int(bool(is_log)), float(conf_scale), _np_ptr(ls), _np_ptr(le), _np_ptr(ws), _np_ptr(we),
                                               _np_ptr(wc), _np_ptr(ps)))
        return Stamps(ls, le, ws, we, wc, ps)

    def ScoreParallel(self, frame_num_utt: Sequence[int], net_out: CuMatrix, hyps: Sequence[Sequence[Sequence[int]]],
                      is_log: bool = False) -> List[np.ndarray]:
        """Exact log-scores ln p(labels | x) (eesen_ctc_score_parallel; INTEGRATION.md "Rescoring").  hyps[s]: any number of labellings
        of utterance s, each a list of class ids in [1, K) (the empty list: the empty labelling).  net_out: posteriors, or log-domain
        scores with is_log=True.  Returns one float32 array per utterance; -1e30 (read <= -1e29) where a labelling has no path.
        Statistics untouched."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        S = fn.size
        if len(hyps) != S:
            raise EesenError(-1, "ScoreParallel: one list of labellings per utterance")
        hoff = np.zeros(S + 1, np.int32)
        hoff[1:] = np.cumsum([len(h) for h in hyps])
        ids, off = self._csr([l for h in hyps for l in h])
        out = np.empty(int(hoff[-1]), np.float32)
        check(self.lib.eesen_ctc_score_parallel(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols, net_out.stride,
                                                int(bool(is_log)), _np_ptr(hoff), _np_ptr(off), _np_ptr(ids), _np_ptr(out) if out.size else None))
        return [out[hoff[s]:hoff[s + 1]] for s in range(S)]

    def RescoreNbest(self, frame_num_utt: Sequence[int], net_out: CuMatrix, is_log: bool = False, lm: Optional["TokenLm"] = None,
                     lm_weight: float = 1.0, bonus: float = 0.0, lm_eos: bool = False) -> "Rescored":
        """Second pass over the entries the last DecodeParallel returned (eesen_ctc_decode_rescore; INTEGRATION.md "Rescoring").
        frame_num_utt, net_out, is_log: that call's.  Every entry gets its exact acoustic score; total = am + lm_weight * g + bonus * n
        with g the fp64 score of `lm` over the entry's n LM tokens (labels, or word ids under a lexicon; lm_eos: with </s>), or, with
        lm=None, the first pass's LM sum.  Returns a Rescored: am_score / lm_score / total [S, nbest] float32 (-1e30 for infeasible
        entries and beyond the returned count), order [S, nbest] int32 -- first-pass ranks by total descending, ties to the smaller
        rank, entries without a score last.  self.hyp and everything else DecodeParallel left keep their first-pass order."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        S = fn.size
        hlen = getattr(self, "hyp_len", None)
        nbest = hlen.shape[1] if hlen is not None and hlen.shape[0] == S else 1   # (without a decode call the library refuses)
        am, lms, tot = (np.empty((S, nbest), np.float32) for _ in range(3))
        order = np.empty((S, nbest), np.int32)
        check(self.lib.eesen_ctc_decode_rescore(self.h, _np_ptr(fn), S, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols, net_out.stride,
                                                int(bool(is_log)), lm.h if lm is not None else None, float(lm_weight), float(bonus),
                                                int(bool(lm_eos)), _np_ptr(am), _np_ptr(lms), _np_ptr(tot), _np_ptr(order)))
        return Rescored(am, lms, tot, order)

    def RescoreTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_rescore_times(self.h, _np_ptr(out)))
        return dict(zip(["lattices", "sweep", "host"], out.tolist()))

    def EditDistanceParallel(self, seqs: Sequence[Sequence[Sequence[int]]], refs: Optional[Sequence[Sequence[int]]] = None):
        """Levenshtein distances on the device (eesen_edit_distance_parallel; INTEGRATION.md "Minimum Bayes risk"), every integer
        equal to edit_distance().  seqs[g]: the sequences of group g, each a list of any int32 tokens.  Returns (pair, ref_dist):
        pair[g] [n_g, n_g] int32, the distances among the group's sequences; ref_dist[g] [n_g] int32, each sequence against
        refs[g] (None without refs).  More than 8192 tokens in a sequence or reference: EESEN_ERR_INVALID.  Statistics untouched."""
        G = len(seqs)
        if refs is not None and len(refs) != G:
            raise EesenError(-1, "EditDistanceParallel: one reference per group")
        soff = np.zeros(G + 1, np.int32)
        soff[1:] = np.cumsum([len(g) for g in seqs])
        ids, off = self._csr([q for g in seqs for q in g])
        nq = int(soff[-1])
        n2 = [len(g) * len(g) for g in seqs]
        pair = np.empty(max(sum(n2), 1), np.int32)
        rd = np.empty(max(nq, 1), np.int32) if refs is not None else None
        rids, roff = self._csr(refs) if refs is not None else (None, None)
        check(self.lib.eesen_edit_distance_parallel(self.h, G, _np_ptr(soff), _np_ptr(off), _np_ptr(ids), _np_ptr(roff) if refs is not None else None,
                                                    _np_ptr(rids) if refs is not None else None, _np_ptr(pair),
                                                    _np_ptr(rd) if refs is not None else None))
        poff = np.concatenate([[0], np.cumsum(n2)]).astype(np.int64)
        pairs = [pair[poff[g]:poff[g + 1]].reshape(len(seqs[g]), len(seqs[g])) for g in range(G)]
        return pairs, ([rd[soff[g]:soff[g + 1]] for g in range(G)] if refs is not None else None)

    def MbrNbest(self, level: int = 0, scale: float = 1.0, totals=None, refs: Optional[Sequence[Sequence[int]]] = None,
                 ref_only: bool = False) -> "Mbr":
        """Minimum Bayes risk over the entries the last DecodeParallel returned (eesen_ctc_decode_mbr; INTEGRATION.md "Minimum Bayes
        risk").  level 0: distances over the mode's LM tokens (labels, or word ids under a lexicon), 1: over labels.  The posterior
        is softmax(scale * z) over the entries that count, z = totals [S, nbest] if given (RescoreNbest's totals) else the decode
        call's scores; risk_i = sum_k P_k d(i, k).  refs[s]: utterance s's reference tokens, for ref_dist.  Returns an Mbr.  ref_only:
        nothing but ref_dist is asked for (no pairwise distances are computed; the other fields are None).  Nothing the decode call
        left is changed."""
        hlen = getattr(self, "hyp_len", None)
        S, nbest = hlen.shape if hlen is not None else (1, 1)   # (without a decode call the library refuses)
        if refs is not None and len(refs) != S:
            raise EesenError(-1, "MbrNbest: one reference per utterance")
        tot = np.ascontiguousarray(totals, np.float32) if totals is not None else None
        if tot is not None and tot.shape != (S, nbest):
            raise EesenError(-1, "MbrNbest: totals must be [S, nbest]")
        rd = np.empty((S, nbest), np.int32) if refs is not None else None
        rids, roff = self._csr(refs) if refs is not None else (None, None)
        if ref_only:
            check(self.lib.eesen_ctc_decode_mbr(self.h, S, int(level), float(scale), _np_ptr(tot) if tot is not None else None,
                                                _np_ptr(roff) if refs is not None else None, _np_ptr(rids) if refs is not None else None,
                                                None, _np_ptr(rd) if refs is not None else None, None, None, None))
            return Mbr(None, rd, None, None, None)
        dist = np.empty((S, nbest, nbest), np.int32)
        post, risk = np.empty((S, nbest), np.float64), np.empty((S, nbest), np.float64)
        order = np.empty((S, nbest), np.int32)
        check(self.lib.eesen_ctc_decode_mbr(self.h, S, int(level), float(scale), _np_ptr(tot) if tot is not None else None,
                                            _np_ptr(roff) if refs is not None else None, _np_ptr(rids) if refs is not None else None,
                                            _np_ptr(dist), _np_ptr(rd) if refs is not None else None, _np_ptr(post), _np_ptr(risk), _np_ptr(order)))
        return Mbr(dist, rd, post, risk, order)

    def MbrTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_mbr_times(self.h, _np_ptr(out)))
        return dict(zip(["build", "kernel", "host"], out.tolist()))

    def SetLmLookahead(self, mode: int):
        """eesen_ctc_set_lm_lookahead: 0 = off (the default), 1 = the unigram look-ahead in the two lexicon searches; it stays set."""
        check(self.lib.eesen_ctc_set_lm_lookahead(self.h, int(mode)))

    def LmLookahead(self) -> int:
        m = C.c_int()
        check(self.lib.eesen_ctc_get_lm_lookahead(self.h, C.byref(m)))
        return m.value

    def SetStampGroup(self, lattices: int):
        """Test hook (eesen_ctc_set_stamp_group): sweep DecodeStamps' lattices in groups of `lattices`; 0 = automatic."""
        check(self.lib.eesen_ctc_set_stamp_group(self.h, int(lattices)))

    def StampTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_stamp_times(self.h, _np_ptr(out)))
        return dict(zip(["lattices", "sweep", "stamps"], out.tolist()))

    def DecodeCandidates(self, rows: int, max_classes: int):
        """The candidate classes the last DecodeParallel selected (tests): (ids [rows, C'], scores [rows, C'], blank [rows])."""
        n = C.c_int(0)
        check(self.lib.eesen_ctc_get_decode_candidates(self.h, None, None, None, C.byref(n)))
        ids = np.empty((rows, n.value), np.int32)
        sc = np.empty((rows, n.value), np.float32)
        bl = np.empty(rows, np.float32)
        check(self.lib.eesen_ctc_get_decode_candidates(self.h, _np_ptr(ids), _np_ptr(sc), _np_ptr(bl), None))
        return ids, sc, bl

    def ErrorRateMSeq(self, frame_num_utt: Sequence[int], net_out: CuMatrix, label: Sequence[Sequence[int]], deferred: bool = False):
        """Ctc::ErrorRateMSeq (ctc-loss.cc:235-298): accumulates the error / reference token counts.  Returns this call's
        (errors, refs); with deferred=True only the argmax and the copy of the ids are enqueued and the host part (collapse +
        edit distance) runs at the next call / stats(), under the device's backward pass -- the reference's call returns void."""
        fn = np.ascontiguousarray(frame_num_utt, np.int32)
        ids, off = self._csr(label)
        ne, nr = C.c_int(), C.c_int()
        check(self.lib.eesen_ctc_error_rate_mseq(self.h, _np_ptr(fn), fn.size, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                                 net_out.stride, _np_ptr(ids), _np_ptr(off), None if deferred else C.byref(ne),
                                                 None if deferred else C.byref(nr)))
        return None if deferred else (ne.value, nr.value)

    def stats(self) -> dict:
        o, s, f, e, r = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long()
        check(self.lib.eesen_ctc_stats(self.h, C.byref(o), C.byref(s), C.byref(f), C.byref(e), C.byref(r)))
        return dict(obj_sum=o.value, sequences=s.value, frames=f.value, err_tokens=e.value, ref_tokens=r.value)

    def NumErrorTokens(self) -> int:
        return self.stats()["err_tokens"]

    def NumRefTokens(self) -> int:
        return self.stats()["ref_tokens"]

    def Report(self) -> str:
        """Ctc::Report (ctc-loss.cc:300-304); train_ctc_parallel.sh greps this line."""
        st = self.stats()
        acc = 100.0 * (1.0 - st["err_tokens"] / st["ref_tokens"]) if st["ref_tokens"] else float("nan")
        return f"\nTOKEN_ACCURACY >> {acc:g}% <<"

    def alpha_beta(self):
        """(alpha, beta) of the last EvalParallel in the reference's [T*S x L'] layout (parity accessor)."""
        L = C.c_int()
        check(self.lib.eesen_ctc_get_alpha_beta(self.h, None, None, C.byref(L)))
        rows = self._rows
        a = np.empty((rows, L.value), np.float32)
        b = np.empty((rows, L.value), np.float32)
        check(self.lib.eesen_ctc_get_alpha_beta(self.h, _np_ptr(a), _np_ptr(b), C.byref(L)))
        return a, b

    def SetGuard(self, net: Optional[Net]):
        """Drop minibatches computed from a timed-out persistent forward pass of `net` from the statistics (eesen_ctc_set_guard)."""
        check(self.lib.eesen_ctc_set_guard(self.h, net.h if net is not None else None))
        self._guard = net

    def Dropped(self) -> int:
        n = C.c_long()
        check(self.lib.eesen_ctc_dropped(self.h, C.byref(n)))
        return n.value

    def SetSequenceOutFile(self, path: Optional[str]):
        """--sequence-out-file (train-ctc-parallel.cc:53-54,134-137): ErrorRateMSeq appends `utt | label frame prob | ...` lines."""
        check(self.lib.eesen_ctc_set_sequence_out_file(self.h, path.encode() if path else None))

    def SetProfiling(self, accumulate: bool):
        """accumulate=True: PhaseTimes() returns the sums over all EvalParallel calls since the last read (no per-call sync)."""
        check(self.lib.eesen_ctc_set_profiling(self.h, 2 if accumulate else 0))

    def PhaseTimes(self) -> dict:
        out = np.zeros(3, np.float32)
        check(self.lib.eesen_ctc_get_phase_times(self.h, _np_ptr(out)))
        return dict(zip(["log", "alpha_beta", "error_diff"], out.tolist()))


class CE:
    """eesen::CE (ce-loss.h:32-77): frame-level cross-entropy over softmax outputs, one fused pass on the device
    (include/eesen_hip.h `eesen_ce_*`)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = _lib.load()
        self.device = device
        self.h = C.c_void_p()
        check(self.lib.eesen_ce_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.obj = None

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_ce_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def EvalParallel(self, net_out: CuMatrix, targets: Sequence[int], diff: Optional[CuMatrix] = None,
                     frame_num_utt: Optional[Sequence[int]] = None, want_obj: bool = True) -> CuMatrix:
        """CE::EvalParallel (ce-loss.cc:94-169): targets = one class id per row t*S + s; row valid iff t < frame_num_utt[s]
        (None: S = 1 and every row valid).  Returns diff = (y - onehot) on valid rows, 0 on padded rows (allocated when not
        given); self.obj = this call's objective.  want_obj=False: nothing waits for the device (self.obj is None then)."""
        fn = np.ascontiguousarray([net_out.rows] if frame_num_utt is None else frame_num_utt, np.int32)
        tg = np.ascontiguousarray(targets, np.int32)
        if tg.size != net_out.rows:
            raise EesenError(-1, f"{tg.size} targets for {net_out.rows} rows")
        if diff is None:
            diff = CuMatrix(net_out.rows, net_out.cols, self.device, zero=False)
        obj = C.c_double()
        check(self.lib.eesen_ce_eval_parallel(self.h, _np_ptr(fn), fn.size, C.c_void_p(net_out.ptr), net_out.rows, net_out.cols,
                                              net_out.stride, _np_ptr(tg), C.c_void_p(diff.ptr), diff.stride,
                                              C.byref(obj) if want_obj else None))
        self.obj = obj.value if want_obj else None
        return diff

    def Eval(self, net_out: CuMatrix, targets: Sequence[int], diff: Optional[CuMatrix] = None) -> CuMatrix:
        """CE::Eval (ce-loss.cc:30-92): one sequence, no mask, sequences += 1."""
        return self.EvalParallel(net_out, targets, diff, None)

    def SetReportStep(self, report_step: int):
        check(self.lib.eesen_ce_set_report_step(self.h, int(report_step)))

    def stats(self) -> dict:
        o, c, f, s = C.c_double(), C.c_long(), C.c_long(), C.c_long()
        check(self.lib.eesen_ce_stats(self.h, C.byref(o), C.byref(c), C.byref(f), C.byref(s)))
        return dict(obj=o.value, correct=c.value, frames=f.value, sequences=s.value)

    def Progress(self, wait: bool = False) -> List[str]:
        """The progress lines of ce-loss.cc:153-167 that are ready (wait=True: after every pending call has arrived)."""
        out, buf = [], C.create_string_buffer(4096)
        while True:
            check(self.lib.eesen_ce_progress(self.h, 1 if wait else 0, buf, len(buf)))
            if not buf.value:
                return out
            out.append(buf.value.decode())

    def Report(self) -> str:
        """CE::Report (ce-loss.cc:171-175), with the true ratio correct / frames (CE)."""
        buf = C.create_string_buffer(256)
        check(self.lib.eesen_ce_report(self.h, buf, len(buf)))
        return buf.value.decode()

    def SetGuard(self, net: Optional[Net]):
        """Drop minibatches computed from a timed-out persistent forward pass of `net` from the statistics (eesen_ce_set_guard)."""
        check(self.lib.eesen_ce_set_guard(self.h, net.h if net is not None else None))
        self._guard = net

    def Dropped(self) -> int:
        n = C.c_long()
        check(self.lib.eesen_ce_dropped(self.h, C.byref(n)))
        return n.value

    def SetProfiling(self, accumulate: bool):
        check(self.lib.eesen_ce_set_profiling(self.h, 2 if accumulate else 0))

    def PhaseTimes(self) -> dict:
        out = np.zeros(1, np.float32)
        check(self.lib.eesen_ce_get_phase_times(self.h, _np_ptr(out)))
        return dict(ce=float(out[0]))


class Feeder:
    """Device-side minibatch assembly, double-buffered (include/eesen_hip.h `eesen_feeder_*`; replaces the host padding +
    interleave + blocking copy of /root/reference/src/netbin/train-ctc-parallel.cc:186-195).

        slot = feeder.submit(mats)          # S host matrices [T_s x D]; returns at once, copy + interleave run async
        feats = feeder.acquire(slot)        # CuMatrix view [T*S x D], row t*S + s; the compute stream waits on-device
        out = net.Propagate(feats); feeder.release(slot)
    """

    def __init__(self, device: int = 0, stream: Optional[int] = None, slots: int = 2):
        self.lib = _lib.load()
        self.device = device
        self.h = C.c_void_p()
        check(self.lib.eesen_feeder_create(device, C.c_void_p(stream) if stream else None, slots, C.byref(self.h)))
        self._dims = {}
        self._batch = {}    # slot -> (utterances, widest boundary) of its batch, for stats()

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_feeder_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def set_pipeline(self, stages: Sequence[Tuple[int, int, int]]):
        """The feature filters of the recipes' rspecifier pipe, run on the device between the PCIe copy and the interleave
        (`eesen_feeder_set_pipeline`; stages = [(EESEN_FEAT_*, a, b)], see eesen_amd.frontend).  Empty list: none."""
        arr = (C.c_int * (3 * max(len(stages), 1)))()
        for i, (k, a, b) in enumerate(stages):
            arr[3 * i], arr[3 * i + 1], arr[3 * i + 2] = int(k), int(a), int(b)
        check(self.lib.eesen_feeder_set_pipeline(self.h, C.cast(arr, C.c_void_p), len(stages)))
        self._has_pipeline = len(stages) > 0

    def set_fbank(self, **opts):
        """Options of the filterbank head stage (`eesen_feeder_set_fbank`; keywords as for `Fbank`), to be called before a
        set_pipeline whose first stage is EESEN_FEAT_FBANK: submit_raw then takes waveforms as [samples x 1] matrices."""
        self._fbank_opts = fbank_opts(**opts)
        check(self.lib.eesen_feeder_set_fbank(self.h, C.byref(self._fbank_opts)))

    def set_pitch(self, **opts):
        """Options of the pitch half of the filterbank + pitch head stage (`eesen_feeder_set_pitch`; keywords as for `Pitch`), to be
        called, like set_fbank, before a set_pipeline whose first stage is EESEN_FEAT_FBANK_PITCH."""
        self._pitch_opts = pitch_opts(**opts)
        check(self.lib.eesen_feeder_set_pitch(self.h, C.byref(self._pitch_opts)))

    def pipeline_shape(self, D_in: int, frames_in: int) -> Tuple[int, int]:
        """(frames, feature dimension) behind the pipeline for an utterance of [frames_in x D_in]."""
        d, t = C.c_int(), C.c_int()
        check(self.lib.eesen_feeder_pipeline_shape(self.h, int(D_in), int(frames_in), C.byref(d), C.byref(t)))
        return t.value, d.value

    def submit_raw(self, mats: Sequence[np.ndarray], cmvn: Optional[Sequence[np.ndarray]] = None) -> int:
        """RAW utterance matrices [T_s x D_in] (+ per utterance the [2 x Dc] CMVN offsets / scales when the pipeline has a
        CMVN stage, None allowed for an utterance without frames); the assembled batch is [T*S x D_out] with T = the longest
        utterance behind the pipeline."""
        if not len(mats):
            raise EesenError(-1, "empty minibatch")
        mats = [np.ascontiguousarray(m, np.float32) for m in mats]
        D = mats[0].shape[1]
        for m in mats:
            if m.ndim != 2 or m.shape[1] != D:
                raise EesenError(-1, f"feature dimension {m.shape[1] if m.ndim == 2 else m.shape} does not match {D}")
        S = len(mats)
        ptrs = (C.c_void_p * S)(*[m.ctypes.data for m in mats])
        frames = np.array([m.shape[0] for m in mats], np.int32)
        cptr = None
        if cmvn is not None:
            if len(cmvn) != S:
                raise EesenError(-1, "one CMVN vector pair per utterance")
            # None: a null pointer, which the library takes for an utterance without frames and refuses for any other
            cmvn = [None if c is None else np.ascontiguousarray(c, np.float32) for c in cmvn]
            given = [c for c in cmvn if c is not None]
            for c in given:
                if c.ndim != 2 or c.shape[0] != 2 or c.shape[1] != given[0].shape[1]:
                    raise EesenError(-1, "CMVN vectors must be [2 x dim] (offsets, scales)")
            cptr = (C.c_void_p * S)(*[None if c is None else c.ctypes.data for c in cmvn])
        slot = C.c_int()
        check(self.lib.eesen_feeder_submit_raw(self.h, ptrs, frames.ctypes.data_as(C.POINTER(C.c_int)), None, cptr, S, D, C.byref(slot)))
        self._dims[slot.value] = self.pipeline_shape(D, 1)[1]
        self._batch[slot.value] = (S, max(D, self._dims[slot.value]))
        return slot.value

    def submit(self, mats: Sequence[np.ndarray]) -> int:
        if not len(mats):
            raise EesenError(-1, "empty minibatch")
        if hasattr(mats[0], "raw"):     # eesen_amd.frontend.RawUtt: raw matrix + CMVN vectors, shape = behind the pipeline
            return self.submit_raw([m.raw for m in mats], [m.cmvn for m in mats] if mats[0].cmvn is not None else None)
        mats = [m if (m.dtype == np.float32 and m.ndim == 2 and m.strides[1] == 4 and m.strides[0] % 4 == 0 and m.strides[0] >= 4 * m.shape[1])
                else np.ascontiguousarray(m, np.float32) for m in mats]
        D = mats[0].shape[1]
        for m in mats:
            if m.ndim != 2 or m.shape[1] != D:
                raise EesenError(-1, f"feature dimension {m.shape[1] if m.ndim == 2 else m.shape} does not match {D}")
        S = len(mats)
        ptrs = (C.c_void_p * S)(*[m.ctypes.data for m in mats])
        frames = np.array([m.shape[0] for m in mats], np.int32)
        strides = np.array([m.strides[0] // 4 for m in mats], np.int32)
        slot = C.c_int()
        check(self.lib.eesen_feeder_submit(self.h, ptrs, frames.ctypes.data_as(C.POINTER(C.c_int)), strides.ctypes.data_as(C.POINTER(C.c_int)),
                                           S, D, C.byref(slot)))
        self._dims[slot.value] = D
        self._batch[slot.value] = (S, D)
        return slot.value

    def acquire(self, slot: int) -> CuMatrix:
        p, T, S, ld = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        check(self.lib.eesen_feeder_acquire(self.h, slot, C.byref(p), C.byref(T), C.byref(S), C.byref(ld)))
        return CuMatrix.view(p.value, T.value * S.value, self._dims[slot], ld.value, self.device, keepalive=self)

    def release(self, slot: int):
        check(self.lib.eesen_feeder_release(self.h, slot))

    def set_stats_tap(self, boundary: int):
        """CMVN statistics of what the pipeline holds at stage boundary `boundary` (0: what was submitted, k: what stage k-1 wrote;
        -1: off), computed beside the batch assembly (`eesen_feeder_set_stats_tap`); read them with `stats(slot)`."""
        check(self.lib.eesen_feeder_set_stats_tap(self.h, int(boundary)))

    def stats(self, slot: int) -> List[np.ndarray]:
        """Per utterance of the batch in `slot` the [2 x (D+1)] float64 statistics at the tapped boundary (`eesen_feeder_stats`)."""
        if slot not in self._dims:
            raise EesenError(-3, "slot holds no submitted batch")
        S, widest = self._batch[slot]     # no stage narrows a matrix: the widest boundary is the first or the last
        buf = np.zeros(S * 2 * (widest + 1), np.float64)
        d = C.c_int()
        check(self.lib.eesen_feeder_stats(self.h, int(slot), buf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(d)))
        n = 2 * (d.value + 1)
        return [buf[s * n:(s + 1) * n].reshape(2, d.value + 1).copy() for s in range(S)]


def cmvn_stats(mats: Sequence[np.ndarray], weights: Optional[Sequence[Optional[np.ndarray]]] = None, device: int = 0,
               stream: Optional[int] = None) -> List[np.ndarray]:
    """CMVN statistics on the device (`eesen_cmvn_stats_parallel`; the reference's AccCmvnStats): per matrix [T_s x D] the
    [2 x (D+1)] float64 matrix of sums, count and sums of squares; weights[s] is None (all ones) or T_s per-frame weights."""
    if not len(mats):
        raise EesenError(-1, "empty minibatch")
    mats = [m if (isinstance(m, np.ndarray) and m.dtype == np.float32 and m.ndim == 2 and m.strides[1] == 4 and m.strides[0] % 4 == 0
                  and m.strides[0] >= 4 * m.shape[1]) else np.ascontiguousarray(m, np.float32) for m in mats]
    D = mats[0].shape[1] if mats[0].ndim == 2 else 0
    for m in mats:
        if m.ndim != 2 or m.shape[1] != D:
            raise EesenError(-1, f"feature dimension {m.shape[1] if m.ndim == 2 else m.shape} does not match {D}")
    S = len(mats)
    ptrs = (C.c_void_p * S)(*[m.ctypes.data for m in mats])
    frames = np.array([m.shape[0] for m in mats], np.int32)
    strides = np.array([m.strides[0] // 4 if m.shape[0] > 1 else max(D, 1) for m in mats], np.int32)
    wptr = None
    if weights is not None:
        if len(weights) != S:
            raise EesenError(-1, "one weight vector (or None) per utterance")
        weights = [None if w is None else np.ascontiguousarray(w, np.float32).reshape(-1) for w in weights]
        for w, m in zip(weights, mats):
            if w is not None and len(w) != m.shape[0]:
                raise EesenError(-1, f"weights have wrong dimension {len(w)} vs. {m.shape[0]}")
        wptr = (C.c_void_p * S)(*[None if w is None else w.ctypes.data for w in weights])
    out = np.zeros((S, 2, D + 1), np.float64)
    check(_lib.load().eesen_cmvn_stats_parallel(device, C.c_void_p(stream) if stream else None, ptrs, frames.ctypes.data_as(C.POINTER(C.c_int)),
                                               strides.ctypes.data_as(C.POINTER(C.c_int)), wptr, S, D, out.ctypes.data_as(C.POINTER(C.c_double))))
    return [out[s].copy() for s in range(S)]


def cmvn_stats_bench(mats: Sequence[np.ndarray], iters: int = 20, device: int = 0) -> float:
    """Average milliseconds of one statistics launch on these matrices (`eesen_cmvn_stats_bench`)."""
    mats = [np.ascontiguousarray(m, np.float32) for m in mats]
    S, D = len(mats), mats[0].shape[1]
    ptrs = (C.c_void_p * S)(*[m.ctypes.data for m in mats])
    frames = np.array([m.shape[0] for m in mats], np.int32)
    ms = C.c_float()
    check(_lib.load().eesen_cmvn_stats_bench(device, None, ptrs, frames.ctypes.data_as(C.POINTER(C.c_int)), S, D, int(iters), C.byref(ms)))
    return ms.value


def paste_feats(inputs: Sequence[Sequence[np.ndarray]], tolerance: int = 0, device: int = 0, stream: Optional[int] = None) -> List[Optional[np.ndarray]]:
    """paste-feats on the device (`eesen_paste_feats`): inputs[j][s] is utterance s of table j (2..4 tables, each of one width);
    returns per utterance the matrices side by side, trimmed to the shortest, or None where the lengths differ by more than
    `tolerance` or a table's matrix is empty (eesen_amd.frontend.paste_frames)."""
    from .frontend import paste_frames
    n = len(inputs)
    if n < 2 or any(len(t) != len(inputs[0]) for t in inputs) or not len(inputs[0]):
        raise EesenError(-1, "paste_feats: 2..4 tables of as many utterances each")
    S = len(inputs[0])
    tabs = [[np.ascontiguousarray(m, np.float32) for m in t] for t in inputs]
    dims = np.zeros(n, np.int32)
    for j, t in enumerate(tabs):
        widths = {m.shape[1] for m in t if m.ndim == 2 and m.shape[0]}
        if any(m.ndim != 2 for m in t) or len(widths) > 1:
            raise EesenError(-1, f"paste_feats: table {j} must hold matrices of one width")
        dims[j] = widths.pop() if widths else max(t[0].shape[1], 1)
    frames = np.array([[m.shape[0] for m in t] for t in tabs], np.int32)
    rows = [paste_frames(frames[:, s], tolerance) for s in range(S)]
    outs = [np.zeros((r, int(dims.sum())), np.float32) if r else None for r in rows]
    tp = [(C.c_void_p * S)(*[m.ctypes.data for m in t]) for t in tabs]
    ip = (C.c_void_p * n)(*[C.cast(p, C.c_void_p).value for p in tp])
    op = (C.c_void_p * S)(*[o.ctypes.data if o is not None else None for o in outs])
    got = np.zeros(S, np.int32)
    check(_lib.load().eesen_paste_feats(device, C.c_void_p(stream) if stream else None, C.cast(ip, C.c_void_p), dims.ctypes.data_as(C.POINTER(C.c_int)), n,
                                        frames.ctypes.data_as(C.POINTER(C.c_int)), S, int(tolerance), C.cast(op, C.c_void_p), got.ctypes.data_as(C.POINTER(C.c_int))))
    assert list(got) == rows
    return outs


def fbank_opts(**kw) -> "_lib.FbankOpts":
    """The defaults of FbankOptions / FrameExtractionOptions / MelBanksOptions (`eesen_fbank_opts_default`) with `kw` on top:
    field names of eesen_fbank_opts_t; `window_type` by name ("povey", ...); booleans as bool or int."""
    o = _lib.FbankOpts()
    check(_lib.load().eesen_fbank_opts_default(C.byref(o)))
    names = {f[0] for f in _lib.FbankOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise EesenError(-1, f"unknown fbank option {k}")
        if k == "window_type" and isinstance(v, str):
            if v not in _lib.WINDOW_TYPES:
                raise EesenError(-1, f"Invalid window type {v}")
            v = _lib.WINDOW_TYPES[v]
        setattr(o, k, int(v) if isinstance(v, (bool, np.bool_)) else v)
    return o


class Fbank:
    """Log-mel filterbank features from waveforms on the device (include/eesen_hip.h `eesen_fbank_*`; the reference's
    compute-fbank-feats, src/feat/feature-fbank.cc).  Waveforms are 1-d arrays in int16 scale.

        fb = Fbank(num_bins=40, dither=0.0)
        frames, dim = fb.shape(len(wave))
        feats = fb.compute([wave_a, wave_b])     # one launch for the minibatch; list of [frames x dim] float32
    """

    def __init__(self, device: int = 0, stream: Optional[int] = None, **opts):
        self.lib = _lib.load()
        self.opts = fbank_opts(**opts)
        self.h = C.c_void_p()
        check(self.lib.eesen_fbank_create(device, C.c_void_p(stream) if stream else None, C.byref(self.opts), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_fbank_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def shape(self, nsamp: int) -> Tuple[int, int]:
        """(frames, dim) for a waveform of nsamp samples: NumFrames in the extractor's edge mode, num_bins + use_energy."""
        t, d = C.c_int(), C.c_int()
        check(self.lib.eesen_fbank_shape(self.h, int(nsamp), C.byref(t), C.byref(d)))
        return t.value, d.value

    def compute(self, waves: Sequence[np.ndarray], utt_ids: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        if not len(waves):
            raise EesenError(-1, "empty minibatch")
        waves = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in waves]
        S = len(waves)
        outs = [np.zeros(self.shape(len(w)), np.float32) for w in waves]
        wp = (C.c_void_p * S)(*[w.ctypes.data for w in waves])
        op = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
        ns = np.array([len(w) for w in waves], np.int32)
        ids = None
        if utt_ids is not None:
            if len(utt_ids) != S:
                raise EesenError(-1, "one utterance id per waveform")
            ids = np.array(utt_ids, np.uint64)
        check(self.lib.eesen_fbank_compute(self.h, wp, ns.ctypes.data_as(C.POINTER(C.c_int)), ids.ctypes.data if ids is not None else None, S, op))
        return outs

    def mel_banks(self):
        return mel_banks(self.opts)


def mel_banks(opts: "_lib.FbankOpts"):
    """(first_index [num_bins], size [num_bins], list of weight vectors) of the reference's MelBanks for `opts` (vtln_warp
    included); host only, no device needed (`eesen_fbank_mel_banks`)."""
    lib = _lib.load()
    nb = max(int(opts.num_bins), 0)
    first, size = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    n = C.c_int()
    check(lib.eesen_fbank_mel_banks(C.byref(opts), first.ctypes.data, size.ctypes.data, None, 0, C.byref(n)))
    w = np.zeros(n.value, np.float32)
    check(lib.eesen_fbank_mel_banks(C.byref(opts), None, None, w.ctypes.data, n.value, None))
    cuts = np.cumsum(size)[:-1]
    return first, size, np.split(w, cuts)


def pitch_opts(**kw) -> "_lib.PitchOpts":
    """The defaults of PitchExtractionOptions and ProcessPitchOptions (`eesen_pitch_opts_default`) with `kw` on top: field names of
    eesen_pitch_opts_t; booleans as bool or int."""
    o = _lib.PitchOpts()
    check(_lib.load().eesen_pitch_opts_default(C.byref(o)))
    names = {f[0] for f in _lib.PitchOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise EesenError(-1, f"unknown pitch option {k}")
        setattr(o, k, int(v) if isinstance(v, (bool, np.bool_)) else v)
    return o


def pitch_lags(opts: "_lib.PitchOpts") -> np.ndarray:
    """The geometric lag grid of SelectLags for `opts`, in seconds; host only (`eesen_pitch_lags`)."""
    lib = _lib.load()
    n = C.c_int()
    check(lib.eesen_pitch_lags(C.byref(opts), None, 0, C.byref(n)))
    lags = np.zeros(n.value, np.float32)
    check(lib.eesen_pitch_lags(C.byref(opts), lags.ctypes.data, n.value, None))
    return lags


class Pitch:
    """Kaldi pitch features from waveforms on the device (include/eesen_hip.h `eesen_pitch_*`; the reference's
    compute-kaldi-pitch-feats and process-kaldi-pitch-feats, src/feat/pitch-functions.cc).  Waveforms are 1-d arrays in int16 scale.

        pt = Pitch(samp_freq=8000.0, delta_pitch_noise_stddev=0.0)
        frames, raw_dim, processed_dim = pt.shape(len(wave))
        raw = pt.compute([wave_a, wave_b])                  # one minibatch; list of [frames x 2] (NCCF, pitch in Hz)
        feats = pt.compute([wave_a, wave_b], process=True)  # post-processed on the device: [frames + delay x processed_dim]
        feats = pt.process(raw)                             # the post-processing alone
    """

    def __init__(self, device: int = 0, stream: Optional[int] = None, **opts):
        self.lib = _lib.load()
        self.opts = pitch_opts(**opts)
        self.h = C.c_void_p()
        check(self.lib.eesen_pitch_create(device, C.c_void_p(stream) if stream else None, C.byref(self.opts), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h:
            try:
                self.lib.eesen_pitch_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def shape(self, nsamp: int) -> Tuple[int, int, int]:
        """(frames, 2, processed columns) for a waveform of nsamp samples; the processed matrix has frames + delay rows."""
        t, r, d = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.eesen_pitch_shape(self.h, int(nsamp), C.byref(t), C.byref(r), C.byref(d)))
        return t.value, r.value, d.value

    def _ids(self, utt_ids, S):
        if utt_ids is None:
            return None
        if len(utt_ids) != S:
            raise EesenError(-1, "one utterance id per waveform")
        return np.array(utt_ids, np.uint64)

    def _rows(self, frames: int, process: bool) -> Tuple[int, int]:
        if not frames:
            return 0, 0
        return (frames + int(self.opts.delay), self.shape(0)[2]) if process else (frames, 2)

    def compute(self, waves: Sequence[np.ndarray], process: bool = False, utt_ids: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        if not len(waves):
            raise EesenError(-1, "empty minibatch")
        waves = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in waves]
        S = len(waves)
        outs = [np.zeros(self._rows(self.shape(len(w))[0], process), np.float32) for w in waves]
        wp = (C.c_void_p * S)(*[w.ctypes.data for w in waves])
        op = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
        ns = np.array([len(w) for w in waves], np.int32)
        caps = np.array([o.size for o in outs], np.int64)
        ids = self._ids(utt_ids, S)
        check(self.lib.eesen_pitch_compute(self.h, wp, ns.ctypes.data_as(C.POINTER(C.c_int)), ids.ctypes.data if ids is not None else None, S,
                                           int(bool(process)), op, caps.ctypes.data, None))
        return outs

    def process(self, raw: Sequence[np.ndarray], utt_ids: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        if not len(raw):
            raise EesenError(-1, "empty minibatch")
        raw = [np.ascontiguousarray(m, np.float32).reshape(-1, 2) for m in raw]
        S = len(raw)
        outs = [np.zeros(self._rows(m.shape[0], True), np.float32) for m in raw]
        rp = (C.c_void_p * S)(*[m.ctypes.data for m in raw])
        op = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
        fr = np.array([m.shape[0] for m in raw], np.int32)
        caps = np.array([o.size for o in outs], np.int64)
        ids = self._ids(utt_ids, S)
        check(self.lib.eesen_pitch_process(self.h, rp, fr.ctypes.data_as(C.POINTER(C.c_int)), ids.ctypes.data if ids is not None else None, S,
                                           op, caps.ctypes.data, None))
        return outs

    def stages(self, wave: np.ndarray) -> dict:
        """DIAGNOSTIC (`eesen_pitch_nccf`): every stage output of one waveform -- down, nccf_pitch, nccf_pov, lags, avg_norm_prod,
        mean_square, fwd, backptr, track, raw, taken, and the counts frames, first_pass_frames, states."""
        wave = np.ascontiguousarray(wave, np.float32).reshape(-1)
        counts = np.zeros(5, np.int32)
        nul = [None] * 11
        check(self.lib.eesen_pitch_nccf(self.h, wave.ctypes.data, len(wave), counts.ctypes.data, *nul))
        F, f1, ns, n2, n1 = (int(v) for v in counts)
        r = dict(frames=F, first_pass_frames=f1, states=ns, down=np.zeros(n2, np.float32), nccf_pitch=np.zeros((F, ns), np.float32),
                 nccf_pov=np.zeros((F, ns), np.float32), lags=np.zeros(ns, np.float32), avg_norm_prod=np.zeros(F, np.float32),
                 mean_square=np.zeros(2, np.float64), fwd=np.zeros(ns, np.float32), backptr=np.zeros((F, ns), np.uint16),
                 track=np.zeros(F, np.int32), raw=np.zeros((F, 2), np.float32), first_pass_samples=n1)
        taken = C.c_int()
        check(self.lib.eesen_pitch_nccf(self.h, wave.ctypes.data, len(wave), counts.ctypes.data, *[r[k].ctypes.data for k in (
            "down", "nccf_pitch", "nccf_pov", "lags", "avg_norm_prod", "mean_square", "fwd", "backptr", "track", "raw")], C.addressof(taken)))
        r["taken"] = bool(taken.value)
        return r

    def lags(self) -> np.ndarray:
        return pitch_lags(self.opts)

    def bench(self, waves: Sequence[np.ndarray], iters: int = 10) -> np.ndarray:
        """Milliseconds per repetition without the copies: [all four launches, down-sampler, NCCF, search, post-processing]."""
        waves = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in waves]
        S = len(waves)
        wp = (C.c_void_p * S)(*[w.ctypes.data for w in waves])
        ns = np.array([len(w) for w in waves], np.int32)
        ms = np.zeros(5, np.float32)
        check(self.lib.eesen_pitch_bench(self.h, wp, ns.ctypes.data_as(C.POINTER(C.c_int)), S, int(iters), ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms


def train_step(net: Net, ctc: Ctc, batch, error_rate: bool = False) -> dict:
    """One pass of the trainer's inner loop (train-ctc-parallel.cc:195-207) on a eesen_amd.synth.Batch."""
    net.SetSeqLengths(batch.lens)
    net_out = net.Propagate(batch.feats)
    diff = ctc.EvalParallel(batch.lens, net_out, batch.labels, getattr(ctc, "_diff", None)
                            if getattr(ctc, "_diff", None) is not None and ctc._diff.rows == net_out.rows and ctc._diff.cols == net_out.cols else None)
    ctc._diff = diff
    ctc._rows = net_out.rows
    res = dict(net_out=net_out, diff=diff, pzx=ctc.pzx)
    if error_rate:
        res["errors"] = ctc.ErrorRateMSeq(batch.lens, net_out, batch.labels)
    net.Backpropagate(diff)
    return res
