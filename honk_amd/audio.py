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

    # -- streams fed tick after tick, their tails and finished rows kept on the device ---------------
    def stream_bank(self, stride, window=16000, front="MFCCs", device=None, slots=64):
        """A ``StreamBank`` of this front end: ``compute_mfccs_segments`` (``front="PCEN"``:
        ``compute_pcen_segments``) for streams that arrive in chunks, fed only their new samples.
        device None: the current ROCm device where there is one, else the CPU.  A shape the plan refuses
        raises ValueError, and on a ROCm device so does a shape a tick would refuse (the mel bands of an MFCC
        bank, the frame-tile kernel's LDS plan): the constructor asks honk_*_bank_tick_i16 itself, with an
        empty tick."""
        return StreamBank(self, stride, window, front, device, slots)

    def _windows_workspace(self, device, nbytes):
        import torch
        key = str(device)
        cache = getattr(self, "_dev_ws", {})
        if key not in cache or cache[key].numel() < nbytes:
            cache[key] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            self._dev_ws = cache
        return cache[key]


BANK_TABLE_ROW = 96  # bytes of a row of a bank tick's table (csrc/mfcc_stream.hip BankRec)


class StreamBank(object):
    """Streams that arrive in chunks, fed only their new samples (honk_*_bank_tick_i16,
    csrc/mfcc_stream.hip; include/honk_hip.h has the contract).  Each open stream owns a slot of device
    memory holding its unconsumed samples and, where windows overlap on whole hops, the finished rows its
    next window reuses.

    ``slot = open()``; ``tick(slot_ids, pcm, offsets) -> (x, window0)`` with ``pcm`` the new samples of the
    fed slots concatenated (1-D int16; a CPU tensor is uploaded once) and stream r's chunk
    ``pcm[offsets[r]:offsets[r + 1]]``: rows ``x[window0[r]:window0[r + 1]]`` are the windows the chunk
    completes -- over any chunking, bit for bit the rows of ``compute_mfccs_windows``
    (``compute_pcen_windows``) on the whole stream.  ``close(slot)`` frees the slot for reuse.  The bank
    doubles when ``open`` runs out of slots.  ``stats``: cumulative ticks, samples_in (samples handed to
    the device), windows, frames_computed, frames_reused.

    On a CPU device the tails are numpy arrays and a tick is ``compute_*_windows`` per stream: the same
    bookkeeping, results and counters (the counters are the plan's arithmetic)."""

    def __init__(self, ap, stride, window=16000, front="MFCCs", device=None, slots=64):
        import torch
        from . import _native
        if front not in ("MFCCs", "PCEN"):
            raise ValueError(f"stream_bank: front {front!r}")
        self.ap, self.stride, self.window, self.front = ap, int(stride), int(window), front
        if self.stride < 1 or self.window < 1 or int(slots) < 1:
            raise ValueError("stream_bank: stride >= 1, window >= 1, slots >= 1")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.pcen = front == "PCEN"
        self.cols = (ap._mel if self.pcen else ap.dct_filters).shape[0]
        self.frames = ap.n_frames(self.window)
        self.plan = _native.StreamBankPlan()
        lib = _native.load()
        rc = lib.honk_stream_bank_plan(self.window, self.stride, ap.n_fft, ap.hop_length, self.cols,
                                       ctypes.addressof(self.plan))
        if rc == 0:  # the front end's own refusals (PCEN: the mel bands, stage 2's tile)
            rc = self._plan(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(1, _native.BANK_SLOT_DTYPE))[0]
        if rc == 0 and self.device.type != "cpu":
            # what only the tick itself knows (the mel bands of an MFCC bank, the frame-tile kernel's LDS plan
            # with its epilogue and group table): an empty tick checks the shape and enqueues nothing
            rc = self._empty_tick()
        if rc != 0:
            raise ValueError("stream_bank: " + lib.honk_last_error().decode(errors="replace"))
        self.route = _native.BANK_ROUTES[self.plan.route]
        self.stats = dict(ticks=0, samples_in=0, windows=0, frames_computed=0, frames_reused=0)
        self._slots = np.zeros(int(slots), _native.BANK_SLOT_DTYPE)
        self._open = np.zeros(int(slots), bool)
        self._tails = {}  # CPU device: slot -> int16 array
        self._state = None
        if self.device.type != "cpu":
            self._state = torch.empty(int(slots) * int(self.plan.slot_bytes), dtype=torch.uint8, device=self.device)

    def _empty_tick(self):
        """honk_*_bank_tick_i16 with no fed stream -> status: the shape checks of a tick and nothing else (no
        pointer is read, nothing is enqueued); host-only."""
        from . import _native
        ap, lib = self.ap, _native.load()
        off = np.zeros(1, np.int64)
        head = (None, None, 0, None, off.ctypes.data, 0, None, 0, None, 0, self.window, self.stride, None, ap.n_fft,
                ap.hop_length, None, ap._mel.shape[0])
        if self.pcen:
            p = ap.pcen_params
            params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
            return lib.honk_pcen_bank_tick_i16(*head, ctypes.addressof(params), None, None, 0, None)
        return lib.honk_mfcc_bank_tick_i16(*head, None, self.cols, None, None, 0, None)

    @property
    def slots(self):
        return len(self._slots)

    def open(self):
        import torch
        free = np.flatnonzero(~self._open)
        if free.size == 0:  # double, existing state preserved
            n = len(self._slots)
            self._slots = np.concatenate([self._slots, np.zeros(n, self._slots.dtype)])
            self._open = np.concatenate([self._open, np.zeros(n, bool)])
            if self._state is not None:
                grown = torch.empty(2 * self._state.numel(), dtype=torch.uint8, device=self.device)
                grown[:self._state.numel()].copy_(self._state)
                self._state = grown
            free = np.flatnonzero(~self._open)
        slot = int(free[0])
        self._open[slot] = True
        self._slots[slot] = (0, 0, 0, 0)
        self._tails.pop(slot, None)
        return slot

    def close(self, slot):
        slot = int(slot)
        if not (0 <= slot < len(self._slots) and self._open[slot]):
            raise ValueError(f"stream_bank: slot {slot} is not open")
        self._open[slot] = False
        self._slots[slot] = (0, 0, 0, 0)
        self._tails.pop(slot, None)

    def _plan(self, ids, off, slots):
        """honk_*_bank_tick_plan -> (status, BankTickPlan, window0, next states, table bytes); host-only."""
        from . import _native
        n = len(ids)
        plan = _native.BankTickPlan()
        window0 = np.zeros(n + 1, np.int64)
        nxt = np.zeros(n, _native.BANK_SLOT_DTYPE)
        table = np.zeros(BANK_TABLE_ROW * (n + 1), np.uint8)
        fn = _native.load().honk_pcen_bank_tick_plan if self.pcen else _native.load().honk_mfcc_bank_tick_plan
        rc = fn(slots.ctypes.data, len(slots), ids.ctypes.data, off.ctypes.data, n, self.window, self.stride,
                self.ap.n_fft, self.ap.hop_length, self.cols, window0.ctypes.data, nxt.ctypes.data, table.ctypes.data,
                table.nbytes, ctypes.addressof(plan))
        return rc, plan, window0, nxt, table

    def tick(self, slot_ids, pcm, offsets):
        import torch
        from . import _native
        if pcm.dim() != 1 or pcm.dtype != torch.int16:
            raise ValueError("stream_bank: pcm must be a 1-D int16 tensor")
        ids = np.ascontiguousarray(np.asarray(slot_ids, dtype=np.int64).reshape(-1))
        off = AudioPreprocessor._segment_offsets("stream_bank", offsets, pcm.shape[0])
        n = len(ids)
        if off.size != n + 1:
            raise ValueError("stream_bank: offsets must have one entry more than slot_ids")
        if ((ids < 0) | (ids >= len(self._slots))).any() or not self._open[ids].all() or len(set(ids.tolist())) != n:
            raise ValueError("stream_bank: slot_ids must be distinct open slots")
        # stride > window: the samples before a stream's next window are dropped here, before any upload
        slots, skip = self._slots, self._slots["skip"][ids]
        if n and (skip > 0).any():
            lens = np.diff(off)
            drop = np.minimum(skip, lens)
            slots = self._slots.copy()   # (committed with the tick)
            slots["skip"][ids] = skip - drop
            parts = [pcm[off[r] + drop[r]:off[r + 1]] for r in range(n)]
            pcm = torch.cat(parts) if parts else pcm[:0]
            off = np.concatenate([[0], np.cumsum(lens - drop)]).astype(np.int64)
        rc, plan, window0, nxt, table = self._plan(ids, off, slots)
        if rc != 0:
            raise ValueError("stream_bank: " + _native.load().honk_last_error().decode(errors="replace"))
        if self._state is None:
            x = self._tick_cpu(ids, pcm, off, plan, nxt)
        else:
            x = self._tick_device(ids, pcm, off, plan, table, slots)
        self._slots = slots
        self._slots[ids] = nxt
        st = self.stats
        st["ticks"] += 1
        for k in ("samples_in", "windows", "frames_computed", "frames_reused"):
            st[k] += int(getattr(plan, k))
        return x, window0

    def _tick_cpu(self, ids, pcm, off, plan, nxt):
        import torch
        windows = self.ap.compute_pcen_windows if self.pcen else self.ap.compute_mfccs_windows
        x = pcm.cpu().numpy()
        parts = []
        for r, slot in enumerate(ids.tolist()):
            buf = np.concatenate([self._tails.get(slot, x[:0]), x[off[r]:off[r + 1]]])
            rows = windows(torch.from_numpy(buf), self.stride, self.window)
            parts.append(rows)
            self._tails[slot] = buf[len(buf) - int(nxt["tail"][r]):].copy()
        out = torch.cat(parts) if parts else torch.empty(0, self.frames, self.cols, dtype=torch.float32)
        assert out.shape[0] == plan.windows
        return out

    def _tick_device(self, ids, pcm, off, plan, table, slots):
        import torch
        from . import _native
        ap, dev = self.ap, self.device
        out = torch.empty(int(plan.windows), self.frames, self.cols, dtype=torch.float32, device=dev)
        if plan.samples_in == 0:
            return out
        chunks = pcm.to(dev).contiguous()
        win, mel, dct = ap._device_tables(dev)
        ws = ap._windows_workspace(dev, plan.workspace_bytes)
        table_dev = torch.from_numpy(table).to(dev)
        head = (chunks.data_ptr(), slots.ctypes.data, len(slots), ids.ctypes.data, off.ctypes.data, len(ids),
                table_dev.data_ptr(), table.nbytes, self._state.data_ptr(), self._state.numel(), self.window,
                self.stride, win.data_ptr(), ap.n_fft, ap.hop_length, mel.data_ptr(), mel.shape[0])
        tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(dev))
        with torch.cuda.device(dev):
            if self.pcen:
                p = ap.pcen_params
                params = _native.PcenParams(p["eps"], p["s"], p["alpha"], p["delta"], p["r"], int(p["power"]))
                rc = _native.load().honk_pcen_bank_tick_i16(*head, ctypes.addressof(params), *tail)
            else:
                rc = _native.load().honk_mfcc_bank_tick_i16(*head, dct.data_ptr(), self.cols, *tail)
        _native.check(rc, "honk_pcen_bank_tick_i16" if self.pcen else "honk_mfcc_bank_tick_i16")
        return out
