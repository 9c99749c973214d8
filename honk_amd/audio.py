"""MFCC front-end: numpy restatement of AudioPreprocessor.compute_mfccs
(/root/reference/utils/manage_audio.py:18-42, librosa 0.6.x semantics).

This is the step before the hot path.  CPU path: numpy
below; ROCm path: ``compute_mfccs_batch`` -> ``honk_mfcc_f32`` (csrc/mfcc.hip).
librosa is not available in this image, so parity of this module is UNPINNED
(checked against the independent float64 restatement oracle/mfcc_ref.py): it restates the
published librosa 0.6 algorithms (STFT with centre/reflect padding and a
periodic Hann window, power spectrum, Slaney mel filterbank with area
normalisation, ``log`` of the positive entries, a 40x40 DCT-II basis from
``librosa.filters.dct``).  Output layout matches the reference: (frames, 40, 1)
float32, which ``collate_fn`` (model.py:258) reshapes to [1, 101, 40].

PCEN front end (``compute_pcen``, manage_audio.py:28,44-47; ``collate_fn``'s other branch,
model.py:253-265): PARITY UNPINNED as well -- the reference's ``pcen`` package
(``StreamingPCENTransform``) is not available, so this restates the published algorithm
(Wang et al. 2017) on the STFT and mel filterbank above:
``E = mel @ |X|^power``; ``M[0] = E[0]``, ``M[t] = (1 - s) M[t-1] + s E[t]`` per band, reset
for every clip; ``out = (E / (M + eps)^alpha + delta)^r - delta^r``, [frames, n_mels], no DCT.
The defaults (``PCEN_DEFAULTS``) follow that package as best they can be restated without it;
pinning its exact choices later changes defaults, not code.  CPU path: numpy
(``compute_pcen``); ROCm path: ``compute_pcen_batch`` -> ``honk_pcen_f32`` (csrc/pcen.hip), and for the
strided windows of one recording ``compute_pcen_windows`` -> ``honk_pcen_windows_i16``.
Checked against the independent float64 restatement tests/pcen_ref.py.
"""
from __future__ import annotations

import ctypes

import numpy as np


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-12) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * m
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), freqs)


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """Slaney-style triangular filters with area normalisation (librosa 0.6 filters.mel, norm=1)."""
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return weights.astype(np.float32)


def dct_filters(n_filters, n_input):
    """librosa 0.6 filters.dct: orthonormal DCT-II basis rows."""
    basis = np.empty((n_filters, n_input))
    basis[0, :] = 1.0 / np.sqrt(n_input)
    samples = np.arange(1, 2 * n_input, 2) * np.pi / (2.0 * n_input)
    for i in range(1, n_filters):
        basis[i, :] = np.cos(i * samples) * np.sqrt(2.0 / n_input)
    return basis


# PCEN parameters (HONK_PCEN_* of include/honk_hip.h); the smoother starts at M[0] = E[0]
PCEN_DEFAULTS = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5, power=1)


class AudioPreprocessor(object):
    def __init__(self, sr=16000, n_dct_filters=40, n_mels=40, f_max=4000, f_min=20, n_fft=480, hop_ms=10,
                 pcen_params=None):
        self.n_mels = n_mels
        self.pcen_params = dict(PCEN_DEFAULTS, **(pcen_params or {}))
        self.dct_filters = dct_filters(n_dct_filters, n_mels)
        self.sr = sr
        self.f_max = f_max if f_max is not None else sr // 2
        self.f_min = f_min
        self.n_fft = n_fft
        self.hop_length = sr // 1000 * hop_ms
        self._mel = mel_filterbank(sr, n_fft, n_mels, f_min, self.f_max)
        n = np.arange(n_fft)
        self._window = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32)

    def n_frames(self, samples):
        """Frames of a centre-padded clip (csrc/mfcc_spectrum.h centre_frames): 1 + samples // hop for
        even n_fft; for odd n_fft the padded clip is one sample shorter than samples + n_fft."""
        return 1 + (int(samples) + 2 * (self.n_fft // 2) - self.n_fft) // self.hop_length

    def _stft(self, y):
        y = np.asarray(y, dtype=np.float32)
        pad = self.n_fft // 2
        y = np.pad(y, (pad, pad), mode="reflect")
        n_frames = 1 + (len(y) - self.n_fft) // self.hop_length
        idx = np.arange(self.n_fft)[None, :] + self.hop_length * np.arange(n_frames)[:, None]
        frames = y[idx] * self._window[None, :]
        return np.fft.rfft(frames, n=self.n_fft, axis=1).astype(np.complex64)  # (frames, bins)

    def melspectrogram(self, y):
        power = (np.abs(self._stft(y)) ** 2).astype(np.float32).T  # (bins, frames)
        return self._mel @ power  # (n_mels, frames)

    def compute_mfccs(self, data):
        data = self.melspectrogram(data)
        pos = data > 0
        data[pos] = np.log(data[pos])
        out = (self.dct_filters @ data).T  # (frames, n_dct)
        return np.asfortranarray(out[:, :, None]).astype(np.float32)

    # -- PCEN (module docstring; PARITY UNPINNED) ------------------------------------
    def _pcen_clip(self, y):
        """y: [S] -> [frames, n_mels] float32."""
        p = self.pcen_params
        if p["power"] not in (1, 2):
            raise ValueError("pcen: power must be 1 or 2")
        mag = np.abs(self._stft(y)).astype(np.float32)
        E = ((mag * mag if p["power"] == 2 else mag) @ self._mel.T).astype(np.float32)  # (frames, n_mels)
        s, a = np.float32(p["s"]), np.float32(1.0) - np.float32(p["s"])
        M = np.empty_like(E)
        M[0] = E[0]
        for t in range(1, E.shape[0]):
            M[t] = a * M[t - 1] + s * E[t]
        r, delta = np.float32(p["r"]), np.float32(p["delta"])
        gain = np.power(M + np.float32(p["eps"]), -np.float32(p["alpha"]))
        return (np.power(E * gain + delta, r) - np.power(np.zeros_like(E) + delta, r)).astype(np.float32)

    def compute_pcen(self, data):
        """data: numpy or CPU torch, [S], [1, S] or [B, S] -> torch float32 [B, frames, n_mels] (the
        reference hands in [1, S] and concatenates along dim 0); the smoother restarts for every clip."""
        import torch
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        data = np.asarray(data, dtype=np.float32)
        if data.ndim == 1:
            data = data[None]
        if data.ndim != 2:
            raise ValueError("compute_pcen: data must be [S], [1, S] or [B, S]")
        frames = self.n_frames(data.shape[1])
        out = np.empty((data.shape[0], frames, self.n_mels), np.float32)
        for i, y in enumerate(data):
            out[i] = self._pcen_clip(y)
        return torch.from_numpy(out)

    def compute_pcen_batch(self, pcm):
        """pcm: torch float32 [B, samples] -> [B, frames, n_mels] on pcm's device: honk_pcen_f32 on a ROCm
        device (chunks of 65535 clips), ``compute_pcen`` on the CPU."""
        import torch
        from . import _native
        if not pcm.is_cuda:
            return self.compute_pcen(pcm)
        pcm = pcm.contiguous().float()
        B, S = pcm.shape
        win, mel, _ = self._device_tables(pcm.device)
        frames = self.n_frames(S)
        out = torch.empty(B, frames, mel.shape[0], dtype=torch.float32, device=pcm.device)
        p = self.pcen_params
        params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
        lib = _native.load()
        with torch.cuda.device(pcm.device):
            for s0 in range(0, B, 65535):
                n = min(65535, B - s0)
                _native.check(lib.honk_pcen_f32(pcm[s0:].data_ptr(), n, S, win.data_ptr(), self.n_fft,
                                                self.hop_length, mel.data_ptr(), mel.shape[0], ctypes.addressof(params),
                                                out[s0:].data_ptr(), _native.stream_handle(pcm.device)),
                              "honk_pcen_f32")
        return out

    # -- batched GPU path (libhonk_hip.so honk_mfcc_f32) ---------------------------
    def _device_tables(self, device):
        import torch
        key = str(device)
        cache = getattr(self, "_dev_tables", {})
        if key not in cache:
            cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(device)
                               for t in (self._window, self._mel, self.dct_filters))
            self._dev_tables = cache
        return cache[key]

    def compute_mfccs_batch(self, pcm):
        """pcm: torch float32 [B, samples] on a ROCm device -> [B, frames, n_dct] (model input layout)."""
        import torch
        from . import _native
        if not pcm.is_cuda:
            return torch.from_numpy(np.stack([self.compute_mfccs(p.numpy()).squeeze(2) for p in pcm]))
        pcm = pcm.contiguous().float()
        B, S = pcm.shape
        win, mel, dct = self._device_tables(pcm.device)
        frames = self.n_frames(S)
        out = torch.empty(B, frames, dct.shape[0], dtype=torch.float32, device=pcm.device)
        lib = _native.load()
        with torch.cuda.device(pcm.device):
            for s0 in range(0, B, 65535):
                n = min(65535, B - s0)
                _native.check(lib.honk_mfcc_f32(pcm[s0:].data_ptr(), n, S, win.data_ptr(), self.n_fft,
                                                self.hop_length, mel.data_ptr(), mel.shape[0], dct.data_ptr(),
                                                dct.shape[0], out[s0:].data_ptr(), _native.stream_handle(pcm.device)),
                              "honk_mfcc_f32")
        return out

    # -- strided windows of one recording (libhonk_hip.so honk_mfcc_windows_i16) ---------
    def windows_plan(self, samples, stride, window=16000, first=0, count=0):
        """honk_mfcc_windows_plan for this front end's n_fft / hop -> (status, MfccWindowsPlan); host-only."""
        import ctypes
        from . import _native
        plan = _native.MfccWindowsPlan()
        rc = _native.load().honk_mfcc_windows_plan(int(samples), int(window), int(stride), self.n_fft,
                                                   self.hop_length, int(first), int(count), ctypes.addressof(plan))
        return rc, plan

    def compute_mfccs_windows(self, pcm, stride, window=16000, first=0, count=None):
        """pcm: 1-D int16 torch tensor, one recording -> [count, frames, n_dct] float32: the MFCC of the
        windows ``pcm[w*stride : w*stride + window] / 32768`` for w in [first, first + count) (count None:
        up to the recording's last whole window), as ``service.stride`` yields them.

        ROCm device: honk_mfcc_windows_i16 (csrc/mfcc_stream.hip; each STFT frame once where
        stride % hop == 0), nothing sliced on the host.  CPU: ``compute_mfccs`` per window."""
        import torch
        from . import _native
        if pcm.dim() != 1 or pcm.dtype != torch.int16:
            raise ValueError("compute_mfccs_windows: pcm must be a 1-D int16 tensor")
        stride, window, first = int(stride), int(window), int(first)
        if stride < 1 or window < 1 or first < 0:
            raise ValueError("compute_mfccs_windows: stride >= 1, window >= 1, first >= 0")
        S = pcm.shape[0]
        W = 0 if S < window else 1 + (S - window) // stride
        count = max(0, W - first) if count is None else int(count)
        if count < 0 or first + count > W:
            raise ValueError(f"compute_mfccs_windows: windows [{first}, {first + count}) of {W}")
        frames, n_dct = self.n_frames(window), self.dct_filters.shape[0]
        if not pcm.is_cuda:
            x = pcm.numpy()
            if count == 0:
                return torch.empty(0, frames, n_dct, dtype=torch.float32)
            return torch.from_numpy(np.stack([
                self.compute_mfccs(x[w * stride:w * stride + window].astype(np.float32) / 32768.).squeeze(2)
                for w in range(first, first + count)]))
        pcm = pcm.contiguous()
        out = torch.empty(count, frames, n_dct, dtype=torch.float32, device=pcm.device)
        if count == 0:
            return out
        rc, plan = self.windows_plan(S, stride, window, first, count)
        if rc == -2:  # HONK_ERR_UNSUPPORTED: a shape outside the kernel's plan -> the per-window kernel
            x = (pcm.float() * (1.0 / 32768.0)).unfold(0, window, stride)[first:first + count]
            return self.compute_mfccs_batch(x.contiguous())
        _native.check(rc, "honk_mfcc_windows_plan")
        win, mel, dct = self._device_tables(pcm.device)
        ws = self._windows_workspace(pcm.device, plan.workspace_bytes)
        with torch.cuda.device(pcm.device):
            rc = _native.load().honk_mfcc_windows_i16(
                pcm.data_ptr(), S, window, stride, first, count, win.data_ptr(), self.n_fft, self.hop_length,
                mel.data_ptr(), mel.shape[0], dct.data_ptr(), n_dct, out.data_ptr(), ws.data_ptr(), ws.numel(),
                _native.stream_handle(pcm.device))
        if rc == -2:
            x = (pcm.float() * (1.0 / 32768.0)).unfold(0, window, stride)[first:first + count]
            return self.compute_mfccs_batch(x.contiguous())
        _native.check(rc, "honk_mfcc_windows_i16")
        return out

    # -- PCEN of the same windows (libhonk_hip.so honk_pcen_windows_i16) ------------------
    def pcen_windows_plan(self, samples, stride, window=16000, first=0, count=0):
        """honk_pcen_windows_plan for this front end's n_fft / hop / n_mels -> (status, MfccWindowsPlan);
        host-only."""
        from . import _native
        plan = _native.MfccWindowsPlan()
        rc = _native.load().honk_pcen_windows_plan(int(samples), int(window), int(stride), self.n_fft,
                                                   self.hop_length, self._mel.shape[0], int(first), int(count),
                                                   ctypes.addressof(plan))
        return rc, plan

    def compute_pcen_windows(self, pcm, stride, window=16000, first=0, count=None):
        """pcm: 1-D int16 torch tensor, one recording -> [count, frames, n_mels] float32: the PCEN
        (``self.pcen_params``) of the windows ``pcm[w*stride : w*stride + window] / 32768`` for w in
        [first, first + count) (count None: up to the recording's last whole window), each with its own
        reflect padding and its own smoother.

        ROCm device: honk_pcen_windows_i16 (csrc/mfcc_stream.hip; the mel energies of each STFT frame
        once where stride % hop == 0, then a scan per window), nothing sliced on the host; a shape the
        call refuses as unsupported goes through ``compute_pcen_batch`` on the unfolded windows.
        CPU: ``compute_pcen`` per window."""
        import torch
        from . import _native
        if pcm.dim() != 1 or pcm.dtype != torch.int16:
            raise ValueError("compute_pcen_windows: pcm must be a 1-D int16 tensor")
        stride, window, first = int(stride), int(window), int(first)
        if stride < 1 or window < 1 or first < 0:
            raise ValueError("compute_pcen_windows: stride >= 1, window >= 1, first >= 0")
        S = pcm.shape[0]
        W = 0 if S < window else 1 + (S - window) // stride
        count = max(0, W - first) if count is None else int(count)
        if count < 0 or first + count > W:
            raise ValueError(f"compute_pcen_windows: windows [{first}, {first + count}) of {W}")
        frames, n_mels = self.n_frames(window), self._mel.shape[0]
        if not pcm.is_cuda:
            x = pcm.numpy()
            if count == 0:
                return torch.empty(0, frames, n_mels, dtype=torch.float32)
            return torch.cat([self.compute_pcen(x[w * stride:w * stride + window].astype(np.float32) / 32768.)
                              for w in range(first, first + count)])
        pcm = pcm.contiguous()
        if count == 0:
            return torch.empty(0, frames, n_mels, dtype=torch.float32, device=pcm.device)

        def per_window():  # HONK_ERR_UNSUPPORTED: a shape outside the kernels' plan -> the per-window kernel
            x = (pcm.float() * (1.0 / 32768.0)).unfold(0, window, stride)[first:first + count]
            return self.compute_pcen_batch(x.contiguous())

        rc, plan = self.pcen_windows_plan(S, stride, window, first, count)
        if rc == -2:
            return per_window()
        _native.check(rc, "honk_pcen_windows_plan")
        win, mel, _ = self._device_tables(pcm.device)
        ws = self._windows_workspace(pcm.device, plan.workspace_bytes)
        out = torch.empty(count, frames, n_mels, dtype=torch.float32, device=pcm.device)
        p = self.pcen_params
        params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
        with torch.cuda.device(pcm.device):
            rc = _native.load().honk_pcen_windows_i16(
                pcm.data_ptr(), S, window, stride, first, count, win.data_ptr(), self.n_fft, self.hop_length,
                mel.data_ptr(), n_mels, ctypes.addressof(params), out.data_ptr(), ws.data_ptr(), ws.numel(),
                _native.stream_handle(pcm.device))
        if rc == -2:
            return per_window()
        _native.check(rc, "honk_pcen_windows_i16")
        return out

    # -- a batch of recordings of ragged length in one call (honk_mfcc_segments_i16 / honk_pcen_segments_i16) --
    @staticmethod
    def _segment_offsets(who, offsets, total=None, check=True):
        off = np.asarray(offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError(f"{who}: offsets must be a 1-D integer sequence of n_rec + 1 entries")
        off = np.ascontiguousarray(off, dtype=np.int64)
        if check and (off[0] < 0 or (np.diff(off) < 0).any() or (total is not None and off[-1] > total)):
            raise ValueError(f"{who}: offsets must be nondecreasing within [0, {total}]")
        return off

    def _segments_plan(self, name, extra, offsets, stride, window):
        from . import _native
        off = self._segment_offsets(name, offsets, check=False)  # (the call itself refuses bad values)
        n_rec = off.size - 1
        window0 = np.zeros(n_rec + 1, np.int64)
        table = np.zeros(6 * (n_rec + 1), np.int64)  # n_rec + 1 rows of six int64 (include/honk_hip.h)
        plan = _native.MfccSegmentsPlan()
        rc = getattr(_native.load(), name)(off.ctypes.data, n_rec, int(window), int(stride), self.n_fft,
                                           self.hop_length, *extra, window0.ctypes.data, table.ctypes.data,
                                           table.nbytes, ctypes.addressof(plan))
        return rc, plan, window0, table

    def segments_plan(self, offsets, stride, window=16000):
        """honk_mfcc_segments_plan for this front end's n_fft / hop -> (status, MfccSegmentsPlan, window0
        [n_rec + 1] int64, the per-recording table as an int64 array to copy to the device); host-only."""
        return self._segments_plan("honk_mfcc_segments_plan", (), offsets, stride, window)

    def pcen_segments_plan(self, offsets, stride, window=16000):
        """honk_pcen_segments_plan: ``segments_plan`` with the PCEN call's workspace; host-only."""
        return self._segments_plan("honk_pcen_segments_plan", (self._mel.shape[0],), offsets, stride, window)

    def _compute_segments(self, which, pcm, offsets, stride, window):
        import torch
        from . import _native
        who = f"compute_{which}_segments"
        if pcm.dim() != 1 or pcm.dtype != torch.int16:
            raise ValueError(f"{who}: pcm must be a 1-D int16 tensor")
        stride, window = int(stride), int(window)
        if stride < 1 or window < 1:
            raise ValueError(f"{who}: stride >= 1, window >= 1")
        off = self._segment_offsets(who, offsets, pcm.shape[0])
        n_rec = off.size - 1
        lens = np.diff(off)
        W = np.where(lens < window, 0, 1 + (lens - window) // stride)
        window0 = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
        mfcc = which == "mfccs"
        windows = self.compute_mfccs_windows if mfcc else self.compute_pcen_windows
        frames, cols = self.n_frames(window), (self.dct_filters if mfcc else self._mel).shape[0]

        def per_recording():
            parts = [windows(pcm[off[r]:off[r + 1]], stride, window) for r in range(n_rec) if W[r]]
            return torch.cat(parts) if parts else torch.empty(0, frames, cols, dtype=torch.float32, device=pcm.device)

        if not pcm.is_cuda:
            return per_recording(), window0
        pcm = pcm.contiguous()
        rc, plan, w0, table = self.segments_plan(off, stride, window) if mfcc else \
            self.pcen_segments_plan(off, stride, window)
        if rc == -2:  # HONK_ERR_UNSUPPORTED: a shape outside the kernel's plan
            return per_recording(), window0
        _native.check(rc, "honk_mfcc_segments_plan" if mfcc else "honk_pcen_segments_plan")
        assert np.array_equal(w0, window0)
        out = torch.empty(int(plan.windows), frames, cols, dtype=torch.float32, device=pcm.device)
        if plan.windows == 0:
            return out, window0
        win, mel, dct = self._device_tables(pcm.device)
        ws = self._windows_workspace(pcm.device, plan.workspace_bytes)
        table_dev = torch.from_numpy(table).to(pcm.device)
        head = (pcm.data_ptr(), pcm.shape[0], off.ctypes.data, n_rec, table_dev.data_ptr(), table.nbytes, window,
                stride, win.data_ptr(), self.n_fft, self.hop_length, mel.data_ptr(), mel.shape[0])
        tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pcm.device))
        with torch.cuda.device(pcm.device):
            if mfcc:
                rc = _native.load().honk_mfcc_segments_i16(*head, dct.data_ptr(), cols, *tail)
            else:
                p = self.pcen_params
                params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
                rc = _native.load().honk_pcen_segments_i16(*head, ctypes.addressof(params), *tail)
        if rc == -2:
            return per_recording(), window0
        _native.check(rc, "honk_mfcc_segments_i16" if mfcc else "honk_pcen_segments_i16")
        return out, window0

    def compute_mfccs_segments(self, pcm, offsets, stride, window=16000):
        """pcm: 1-D int16 torch tensor holding a batch of recordings, recording r being
        ``pcm[offsets[r]:offsets[r + 1]]`` (offsets: n_rec + 1 nondecreasing ints within the tensor)
        -> (x [sum W_r, frames, n_dct] float32, window0 [n_rec + 1] int64): recording r's rows
        ``x[window0[r]:window0[r + 1]]`` are ``compute_mfccs_windows`` of that recording alone, bit for bit.

        ROCm device: one plan, one upload of the per-recording table and one honk_mfcc_segments_i16
        (csrc/mfcc_stream.hip), whatever the number of recordings; a shape the call refuses as unsupported
        goes through ``compute_mfccs_windows`` per recording.  CPU: ``compute_mfccs_windows`` per
        recording.  A bad ``offsets`` raises ValueError."""
        return self._compute_segments("mfccs", pcm, offsets, stride, window)

    def compute_pcen_segments(self, pcm, offsets, stride, window=16000):
        """``compute_mfccs_segments`` under PCEN (``self.pcen_params``; honk_pcen_segments_i16):
        recording r's rows are ``compute_pcen_windows`` of that recording alone, bit for bit."""
        return self._compute_segments("pcen", pcm, offsets, stride, window)

    def _windows_workspace(self, device, nbytes):
        import torch
        key = str(device)
        cache = getattr(self, "_dev_ws", {})
        if key not in cache or cache[key].numel() < nbytes:
            cache[key] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            self._dev_ws = cache
        return cache[key]
