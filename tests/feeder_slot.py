"""Helpers of the GPU tests that read a feeder slot's WHOLE assembled matrix, pad columns included (tests/test_gpu_fbank.py,
tests/test_gpu_feeder_fullsize.py)."""
import numpy as np


def slot_matrix(f, slot):
    """The whole assembled matrix of a slot, pad columns included."""
    from eesen_amd.api import CuMatrix
    got = f.acquire(slot)
    host = CuMatrix.view(got.ptr, got.rows, got.stride, got.stride, got.device, keepalive=f).numpy()
    f.release(slot)
    return host


def assembled(mats, ld):
    """The feeder's [T*S x ld] matrix of these utterances: row t*S + s, zeros past an utterance's end and in the pad columns."""
    T, S = max(m.shape[0] for m in mats), len(mats)
    out = np.zeros((T, S, ld), np.float32)
    for s, m in enumerate(mats):
        out[:m.shape[0], s, :m.shape[1]] = m
    return out.reshape(T * S, ld)


def same_bits(host, mats):
    exp = assembled(mats, host.shape[1])
    return host.shape == exp.shape and np.array_equal(host.view(np.uint32), exp.view(np.uint32))
