"""Serving callers of the hot path: LabelService / TorchLabelService / stride
(/root/reference/service.py:28-110).

``TorchLabelService.label(wav_bytes)`` is the batch-1 serving surface: int16 PCM
-> MFCC [1, 101, 40] -> model -> softmax -> (label, prob).  With the model on a
ROCm device the forward runs on the gfx950 kernels.  ``label_batch`` is the
batched form (every window of a request in one forward).
"""
from __future__ import annotations

import os
import warnings
import wave

import numpy as np
import torch
import torch.nn.functional as F

from . import model
from .audio import AudioPreprocessor


def _softmax(x):
    return np.exp(x) / np.sum(np.exp(x))


class LabelService(object):
    def evaluate(self, speech_dirs, indices=[]):
        """service.py:32-50: accuracy of label() over folders of 1 s wav clips."""
        dir_labels = {}
        if indices:
            real_labels = [self.labels[i] for i in indices]
        else:
            real_labels = [os.path.dirname(d) for d in speech_dirs]
        for i, label in enumerate(real_labels):
            if label not in self.labels:
                real_labels[i] = "_unknown_"
            dir_labels[speech_dirs[i]] = real_labels[i]
        accuracy = []
        for folder in speech_dirs:
            for filename in os.listdir(folder):
                with wave.open(os.path.join(folder, filename)) as f:
                    b_data = f.readframes(16000)
                label, _ = self.label(b_data)
                accuracy.append(int(label == dir_labels[folder]))
        return sum(accuracy) / len(accuracy)

    def label(self, wav_data):
        raise NotImplementedError


# the models with honk_schedule and honk_capture
_SCHEDULED = (model.SpeechResModel, model.SpeechModel)


class TorchLabelService(LabelService):
    """service.py:72-104 (hard-wired cnn-trad-pool2, like the reference).

    ``honk_graph`` (opt-in, default False): with the model on a ROCm device (the ``SpeechModel``
    ``reload()`` builds, or a ``SpeechResModel`` put in its place), ``label()`` replays a captured
    batch-1 forward (the model's ``honk_capture``, captured at the first call) instead of
    launching the forward's kernels one by one; ``reload()`` drops the capture.

    ``honk_latency`` (opt-in, default False): ``label()``, ``label_batch()``, ``label_stream()`` (and a
    ``StreamListener`` on this service) run the model's latency schedule (``honk_schedule =
    "latency"``: a small batch split over all CUs -- a ``SpeechResModel``'s logits bit for bit, a
    ``SpeechModel``'s within the 1e-4 bar); with ``honk_graph``, ``label()`` replays a capture of
    that schedule.

    ``audio_preprocess_type`` ("MFCCs", the default, or "PCEN"): the front end the checkpoint was
    trained with (the reference's ``--audio_preprocess_type``).  PCEN restarts its smoother for every
    window, as the reference's ``compute_pcen`` resets its transform after every clip;
    ``label_stream`` (and ``listen_stream`` / a ``StreamListener``) shares the STFT frames' mel energies
    among the windows of a recording as the MFCC path shares its frames (``compute_pcen_windows``).

    Many recordings at once: ``label_streams`` (one upload, one ragged-batch front-end call, one forward
    and one download per batch of windows) and a ``StreamPool`` over it, under either front end."""

    honk_graph = False
    honk_latency = False

    def __init__(self, model_filename, no_cuda=False, labels=["_silence_", "_unknown_", "command", "random"],
                 audio_processor=None, honk_graph=False, audio_preprocess_type="MFCCs", honk_latency=False):
        if audio_preprocess_type not in ("MFCCs", "PCEN"):
            raise ValueError(f"TorchLabelService: audio_preprocess_type {audio_preprocess_type!r}")
        self.audio_preprocess_type = audio_preprocess_type
        self.honk_graph = honk_graph
        self.honk_latency = honk_latency
        self.labels = labels
        self.model_filename = model_filename
        self.no_cuda = no_cuda
        self.audio_processor = audio_processor or AudioPreprocessor()
        self.reload()

    def reload(self):
        self._honk_captured = self._honk_cnn_captured = None
        config = model.find_config(model.ConfigType.CNN_TRAD_POOL2)
        config["n_labels"] = len(self.labels)  # mutates the shared dict, as service.py:82 does
        self.model = model.SpeechModel(config)
        if not self.no_cuda:
            self.model.cuda()
        self.model.load(self.model_filename)
        self.model.eval()

    def _model_input(self, windows):
        """int16 PCM byte windows -> [B, frames, 40] MFCC (or PCEN) on the model's device.

        ROCm: one batched honk_mfcc_f32 / honk_pcen_f32 call (csrc/mfcc.hip, csrc/pcen.hip); CPU: numpy."""
        pcm = np.stack([np.frombuffer(w, dtype=np.int16) for w in windows]).astype(np.float32) / 32768.
        if self.audio_preprocess_type == "PCEN":
            if self.no_cuda:
                return self.audio_processor.compute_pcen(pcm)
            return self.audio_processor.compute_pcen_batch(torch.from_numpy(pcm).cuda())
        if self.no_cuda:
            return torch.from_numpy(np.stack([self.audio_processor.compute_mfccs(p).squeeze(2) for p in pcm]))
        return self.audio_processor.compute_mfccs_batch(torch.from_numpy(pcm).cuda())

    def _net(self):
        """self.model, on the latency schedule where honk_latency asks for it."""
        m = self.model
        if self.honk_latency and isinstance(m, _SCHEDULED) and m.honk_schedule != "latency":
            m.honk_schedule = "latency"
            self._honk_captured = self._honk_cnn_captured = None  # (a capture holds the schedule it was made with)
        return m

    def _forward1(self, model_in):
        """The model's forward of label()'s batch-1 input: the captured one where honk_graph asks for it."""
        m = self._net()
        if not (self.honk_graph and isinstance(m, _SCHEDULED) and model_in.is_cuda and not m.training):
            return m(model_in)
        # (model, CapturedForward): a res model's in _honk_captured, a SpeechModel's in _honk_cnn_captured
        slot = "_honk_captured" if isinstance(m, model.SpeechResModel) else "_honk_cnn_captured"
        cap = getattr(self, slot, None)
        if cap is None or cap[0] is not m or tuple(cap[1].x.shape) != tuple(model_in.shape):
            cap = (m, m.honk_capture(model_in))
            setattr(self, slot, cap)
        return cap[1].replay(model_in)

    def label(self, wav_data):
        """Labels audio data as one of the trained labels -> (most likely label, probability)."""
        model_in = self._model_input([wav_data])
        with torch.no_grad():
            predictions = F.softmax(self._forward1(model_in).squeeze(0).cpu(), dim=0).numpy()
        return (self.labels[np.argmax(predictions)], np.max(predictions))

    def label_batch(self, windows):
        """All windows of a request in ONE MFCC launch + ONE forward; [(label, prob)] in order."""
        if not windows:
            return []
        with torch.no_grad():
            p = F.softmax(self._net()(self._model_input(windows)).cpu(), dim=1).numpy()
        return [(self.labels[int(np.argmax(r))], float(np.max(r))) for r in p]

    def listen(self, wav_data, stride_size_ms=500, method="labels", keyword="command", min_keyword_prob=0.85):
        """Batched form of server.py:99-112 (ListenEndpoint.POST): 1 s windows every
        ``stride_size_ms``; returns {label: summed prob} or, for "command_tagging",
        {"contains_command": bool} with the reference's early-exit order."""
        windows = list(stride(wav_data, int(2 * 16000 * stride_size_ms / 1000), 2 * 16000))
        labels = {}
        for label, prob in self.label_batch(windows):
            labels[label] = labels.get(label, 0.0) + float(prob)
            if label == keyword and prob >= min_keyword_prob and method == "command_tagging":
                return dict(contains_command=True)
        return dict(contains_command=False) if method == "command_tagging" else labels


    def label_stream(self, wav_data, stride_size_ms=500, max_windows=8192):
        """[(label, prob)] of every 1 s window at ``stride_size_ms`` of a recording, in order:
        ``label_batch(list(stride(...)))`` with the front end on the device.  The int16 bytes are
        uploaded once; the windows go through ``compute_mfccs_windows`` (each STFT frame computed
        once), the model's forward and the softmax ``max_windows`` at a time, so memory stays
        bounded whatever the recording's length.  Under PCEN the windows go through
        ``compute_pcen_windows``: the mel energies of each STFT frame once, then every window its own
        smoother; no float copy of the windows is built."""
        stride_bytes = int(2 * 16000 * stride_size_ms / 1000)
        if stride_bytes < 1:
            raise ValueError("label_stream: stride_size_ms too small")
        if self.no_cuda or stride_bytes % 2:
            return self.label_batch(list(stride(wav_data, stride_bytes, 2 * 16000)))
        if max_windows < 1:
            raise ValueError("label_stream: max_windows >= 1")
        n = len(wav_data) // 2
        total = 0 if n < 16000 else 1 + (n - 16000) // (stride_bytes // 2)
        if total == 0:
            return []
        device = next(self.model.parameters()).device
        pcm = torch.from_numpy(np.frombuffer(wav_data, dtype=np.int16, count=n).copy()).to(device)
        out = []
        with torch.no_grad():
            for w0 in range(0, total, max_windows):
                nw = min(max_windows, total - w0)
                if self.audio_preprocess_type == "PCEN":
                    x = self.audio_processor.compute_pcen_windows(pcm, stride_bytes // 2, 16000, w0, nw)
                else:
                    x = self.audio_processor.compute_mfccs_windows(pcm, stride_bytes // 2, 16000, w0, nw)
                p = F.softmax(self._net()(x).cpu(), dim=1).numpy()
                out.extend((self.labels[int(np.argmax(r))], float(np.max(r))) for r in p)
        return out

    def label_streams(self, recordings, stride_size_ms=500, max_windows=8192):
        """``[label_stream(r, stride_size_ms) for r in recordings]`` (int16 byte strings) with the whole
        batch in one front-end call: the bytes are concatenated and uploaded once; the recordings go, in
        order, in batches of at most ``max_windows`` windows through ``compute_mfccs_segments``
        (``compute_pcen_segments`` under PCEN), one forward, one softmax and one download per batch.  A
        recording with more than ``max_windows`` windows goes through ``label_stream`` itself.  On the
        CPU, or with an odd stride in bytes, it is ``label_stream`` per recording."""
        stride_bytes = int(2 * 16000 * stride_size_ms / 1000)
        if stride_bytes < 1:
            raise ValueError("label_streams: stride_size_ms too small")
        if self.no_cuda or stride_bytes % 2:
            return [self.label_stream(r, stride_size_ms, max_windows) for r in recordings]
        if max_windows < 1:
            raise ValueError("label_streams: max_windows >= 1")
        step = stride_bytes // 2
        ns = [len(r) // 2 for r in recordings]
        Ws = [0 if n < 16000 else 1 + (n - 16000) // step for n in ns]
        out = [[] for _ in recordings]
        batched = [i for i, w in enumerate(Ws) if 0 < w <= max_windows]
        for i, w in enumerate(Ws):
            if w > max_windows:
                out[i] = self.label_stream(recordings[i], stride_size_ms, max_windows)
        if not batched:
            return out
        device = next(self.model.parameters()).device
        off = np.concatenate([[0], np.cumsum([ns[i] for i in batched])]).astype(np.int64)
        pcm = torch.from_numpy(np.concatenate([np.frombuffer(recordings[i], dtype=np.int16, count=ns[i])
                                               for i in batched])).to(device)
        segments = self.audio_processor.compute_pcen_segments if self.audio_preprocess_type == "PCEN" else \
            self.audio_processor.compute_mfccs_segments
        with torch.no_grad():
            a = 0
            while a < len(batched):
                b, nw = a, 0
                while b < len(batched) and nw + Ws[batched[b]] <= max_windows:
                    nw += Ws[batched[b]]
                    b += 1
                x, w0 = segments(pcm, off[a:b + 1], step, 16000)
                p = F.softmax(self._net()(x).cpu(), dim=1).numpy()
                for j in range(a, b):
                    out[batched[j]] = [(self.labels[int(np.argmax(r))], float(np.max(r)))
                                       for r in p[w0[j - a]:w0[j - a + 1]]]
                a = b
        return out

    def listen_stream(self, wav_data, stride_size_ms=500, method="labels", keyword="command", min_keyword_prob=0.85):
        """``listen`` over ``label_stream``: the same return contract and early-exit order."""
        labels = {}
        for label, prob in self.label_stream(wav_data, stride_size_ms):
            labels[label] = labels.get(label, 0.0) + float(prob)
            if label == keyword and prob >= min_keyword_prob and method == "command_tagging":
                return dict(contains_command=True)
        return dict(contains_command=False) if method == "command_tagging" else labels


class StreamListener(object):
    """Incremental ``label_stream``: ``feed(wav_bytes)`` returns the (label, prob) of the windows the
    bytes fed so far complete, in order; any chunking of a recording into ``feed`` calls yields the
    windows of ``label_stream`` on the whole recording.  Between calls it keeps only the unconsumed
    tail (less than one window plus one stride)."""

    def __init__(self, service, stride_size_ms=500):
        self.service = service
        self.stride_size_ms = stride_size_ms
        self._stride = int(2 * 16000 * stride_size_ms / 1000)
        self._window = 2 * 16000
        self._buf = b""
        self._skip = 0  # bytes before the next window's start still to come (stride > window)

    def _push(self, wav_bytes):
        """Take in a chunk -> the buffer whose whole windows are to be labelled now, or None while it holds
        less than one window.  The window arithmetic of ``feed`` (and of a ``StreamPool``'s streams)."""
        wav_bytes = bytes(wav_bytes)
        if self._skip:
            drop = min(self._skip, len(wav_bytes))
            self._skip -= drop
            wav_bytes = wav_bytes[drop:]
        self._buf += wav_bytes
        return self._buf if len(self._buf) >= self._window else None

    def _pop(self, labelled):
        """Drop what the ``labelled`` windows of the buffer ``_push`` returned have consumed."""
        done = 1 + (len(self._buf) - self._window) // self._stride
        assert labelled == done
        nxt = done * self._stride
        self._skip = max(0, nxt - len(self._buf))
        self._buf = self._buf[nxt:]

    def feed(self, wav_bytes):
        buf = self._push(wav_bytes)
        if buf is None:
            return []
        out = self.service.label_stream(buf, self.stride_size_ms)
        self._pop(len(out))
        return out


class StreamPool(object):
    """Many ``StreamListener``s on one service, labelled together: ``feed({key: wav_bytes, ...})`` returns
    ``{key: [(label, prob), ...]}`` for every key fed -- per key, over any sequence of ticks, what a
    ``StreamListener`` fed the same bytes returns.  A key is opened at its first feed; ``close(key)`` drops
    its tail.  Per tick the streams that complete at least one window go through ONE
    ``service.label_streams`` call (one upload, one front-end call, one forward, one download), whatever
    their number.  Tails stay on the host, as a ``StreamListener``'s.

    ``device_state=True`` (a ROCm service, an even stride in bytes): a key owns a slot of a
    ``StreamBank`` instead -- its tail and the finished rows its next window reuses stay on the device.
    ``feed`` uploads only the fed bytes and runs one bank tick, the forward in slices of at most 8192
    windows, one softmax and one download.  A chunk that ends mid-sample leaves its odd byte on the host, in
    front of that key's next chunk.  Where the bank cannot be built (a CPU service, an odd stride in bytes,
    a shape its plan or its tick refuses: ``stream_bank`` raises ValueError for both at construction) the
    pool warns once and works as with ``device_state=False``."""

    MAX_WINDOWS = 8192

    def __init__(self, service, stride_size_ms=500, device_state=False):
        self.service = service
        self.stride_size_ms = stride_size_ms
        self._streams = {}
        self.bank = self._make_bank() if device_state else None

    def _make_bank(self):
        svc = self.service
        stride_bytes = int(2 * 16000 * self.stride_size_ms / 1000)
        why = None
        if svc.no_cuda:
            why = "the service runs on the CPU"
        elif stride_bytes < 2 or stride_bytes % 2:
            why = f"a stride of {stride_bytes} bytes is no whole number of samples"
        else:
            try:
                return svc.audio_processor.stream_bank(stride_bytes // 2, 16000, svc.audio_preprocess_type,
                                                       next(svc.model.parameters()).device)
            except ValueError as e:
                why = str(e)
        warnings.warn(f"StreamPool: device_state=True not available ({why}); tails stay on the host")
        return None

    def keys(self):
        return list(self._streams)

    def close(self, key):
        st = self._streams.pop(key, None)
        if self.bank is not None and st is not None:
            self.bank.close(st[0])

    def feed(self, chunks):
        if self.bank is not None:
            return self._feed_bank(chunks)
        out, ready = {}, []
        for key, wav_bytes in chunks.items():
            sl = self._streams.get(key)
            if sl is None:
                sl = self._streams[key] = StreamListener(self.service, self.stride_size_ms)
            out[key] = []
            buf = sl._push(wav_bytes)
            if buf is not None:
                ready.append((key, sl, buf))
        if ready:
            labelled = self.service.label_streams([buf for _, _, buf in ready], self.stride_size_ms)
            for (key, sl, _), got in zip(ready, labelled):
                sl._pop(len(got))
                out[key] = got
        return out

    def _feed_bank(self, chunks):
        """One tick on the bank: a stream is [slot, the odd byte of its last chunk]."""
        svc, out, ids, parts = self.service, {}, [], []
        for key, wav_bytes in chunks.items():
            st = self._streams.get(key)
            if st is None:
                st = self._streams[key] = [self.bank.open(), b""]
            data = st[1] + bytes(wav_bytes)
            n = len(data) // 2
            st[1] = data[2 * n:]
            out[key] = []
            ids.append(st[0])
            parts.append(np.frombuffer(data, dtype=np.int16, count=n))
        if not ids:
            return out
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        x, w0 = self.bank.tick(ids, torch.from_numpy(np.concatenate(parts)), off)
        if x.shape[0]:
            with torch.no_grad():
                net = svc._net()
                logits = torch.cat([net(x[a:a + self.MAX_WINDOWS]) for a in range(0, x.shape[0], self.MAX_WINDOWS)])
                p = F.softmax(logits.cpu(), dim=1).numpy()
            for j, key in enumerate(chunks):
                out[key] = [(svc.labels[int(np.argmax(r))], float(np.max(r))) for r in p[w0[j]:w0[j + 1]]]
        return out


def stride(array, stride_size, window_size):
    """service.py:106-110: sliding windows (server.py:104 uses 0.5 s stride, 1 s window)."""
    i = 0
    while i + window_size <= len(array):
        yield array[i:i + window_size]
        i += stride_size
