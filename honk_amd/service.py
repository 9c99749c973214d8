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


_NUMPY_OF = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}


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
    and one download per batch of windows) and a ``StreamPool`` over it, under either front end.

    ``decide`` is the stage after the forward -- per window the label and its probability, per segment of
    windows the summed probabilities, the counts and the first keyword hit -- as one native call
    (honk_listen_decide_f32, csrc/listen.hip) and one small download; ``listen_streams`` answers a batch of
    recordings from it.  ``honk_decide`` (opt-in, default False): ``label_batch``, ``label_stream``,
    ``label_streams`` and a ``StreamPool`` take their (label, prob) from ``decide`` instead of downloading the
    logits and running softmax / argmax / max row by row on the host."""

    honk_graph = False
    honk_latency = False
    honk_decide = False

    def __init__(self, model_filename, no_cuda=False, labels=["_silence_", "_unknown_", "command", "random"],
                 audio_processor=None, honk_graph=False, audio_preprocess_type="MFCCs", honk_latency=False,
                 honk_decide=False):
        if audio_preprocess_type not in ("MFCCs", "PCEN"):
            raise ValueError(f"TorchLabelService: audio_preprocess_type {audio_preprocess_type!r}")
        self.audio_preprocess_type = audio_preprocess_type
        self.honk_graph = honk_graph
        self.honk_latency = honk_latency
        self.honk_decide = honk_decide
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

    def decide(self, logits, window0=None, keyword=None, min_keyword_prob=0.85):
        """The stage after the forward, on logits [N, n_labels] -> numpy ``(label int32 [N], prob float32
        [N])``: what softmax -> np.argmax / np.max give per row (the first index of the largest logit and
        its probability; a row whose softmax is NaN -- a NaN, a +inf, nothing above -inf -- gives label 0,
        prob NaN).  With ``window0`` (int64 [S + 1], starting at 0, non-decreasing, ending at N: the layout
        ``compute_*_segments`` and ``StreamBank.tick`` return) also ``(sums float64 [S, n_labels], counts
        int32 [S, n_labels], hit int64 [S])`` over segment s = rows ``window0[s]:window0[s + 1]``: the summed
        prob and the number of its rows per label, and the segment-relative index of the first row labelled
        ``keyword`` (a label's name or index; None: no keyword) with ``prob >= min_keyword_prob``, else -1.
        A finite prob is a multiple of 2^-29 within [2^-6, 1] up to 64 labels, so the sums are exact in
        double whatever the order they are taken in.

        A ROCm tensor of at most 64 labels: one honk_listen_decide_f32 (csrc/listen.hip) and ONE download, of
        these small arrays (not of the logits).  Otherwise (a CPU tensor, more labels): the same definition
        with torch's softmax and numpy."""
        from . import _native
        if logits.dim() != 2:
            raise ValueError("decide: logits must be [N, n_labels]")
        n, n_labels = logits.shape
        if keyword is None:
            kw = -1
        elif isinstance(keyword, str):
            kw = self.labels.index(keyword) if keyword in self.labels else -1
        else:
            kw = int(keyword)
        w0 = None if window0 is None else _native.listen_window0(window0, n, "decide")
        if (logits.is_cuda and logits.dtype == torch.float32 and 1 <= n_labels <= _native.LISTEN_MAX_LABELS
                and n <= _native.LISTEN_MAX_WINDOWS):
            parts = _native.listen_decide(logits, w0, kw, min_keyword_prob)
            # one download: the 8-byte arrays first, so every view below is aligned
            order = [parts[i] for i in ((2, 4, 0, 1, 3) if w0 is not None else (0, 1))]
            raw = torch.cat([t.reshape(-1).view(torch.uint8) for t in order]).cpu().numpy()
            got, at = [], 0
            for t in order:
                nb = t.numel() * t.element_size()
                got.append(raw[at:at + nb].view(_NUMPY_OF[t.dtype]).reshape(tuple(t.shape)))
                at += nb
            if w0 is None:
                return got[0], got[1]
            return got[2], got[3], got[0], got[4], got[1]
        with torch.no_grad():
            p = F.softmax(logits.detach().cpu().float(), dim=1).numpy()
        label = np.argmax(p, axis=1).astype(np.int32) if n else np.zeros(0, np.int32)
        prob = np.max(p, axis=1) if n else np.zeros(0, np.float32)
        if w0 is None:
            return label, prob
        segments = w0.size - 1
        seg = np.repeat(np.arange(segments), np.diff(w0))
        p64 = prob.astype(np.float64)
        sums = np.zeros((segments, n_labels), np.float64)
        counts = np.zeros((segments, n_labels), np.int32)
        np.add.at(sums, (seg, label), p64)   # in row order: the host loop's sums
        np.add.at(counts, (seg, label), 1)
        first = np.full(segments, n, np.int64)
        rows = np.flatnonzero((label == kw) & (p64 >= min_keyword_prob)) if kw >= 0 else np.zeros(0, np.int64)
        np.minimum.at(first, seg[rows], rows - w0[seg[rows]])
        return label, prob, sums, counts, np.where(first == n, -1, first)

    def _labelled(self, logits):
        """[(label, prob)] of the rows of ``logits``: the logits downloaded, softmax and argmax / max row by
        row on the host -- or, under ``honk_decide``, both from ``decide``."""
        if self.honk_decide:
            label, prob = self.decide(logits)
            return list(zip(np.asarray(self.labels, dtype=object)[label].tolist(), prob.astype(np.float64).tolist()))
        p = F.softmax(logits.cpu(), dim=1).numpy()
        return [(self.labels[int(np.argmax(r))], float(np.max(r))) for r in p]

    def label_batch(self, windows):
        """All windows of a request in ONE MFCC launch + ONE forward; [(label, prob)] in order."""
        if not windows:
            return []
        with torch.no_grad():
            return self._labelled(self._net()(self._model_input(windows)))

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
        stride_bytes = self._stride_bytes("label_stream", stride_size_ms, max_windows)
        out = []
        for logits in self._recording_logits(wav_data, stride_bytes, max_windows):
            out.extend(self._labelled(logits))
        return out

    def _stride_bytes(self, who, stride_size_ms, max_windows):
        stride_bytes = int(2 * 16000 * stride_size_ms / 1000)
        if stride_bytes < 1:
            raise ValueError(f"{who}: stride_size_ms too small")
        if max_windows < 1 and not (self.no_cuda or stride_bytes % 2):
            raise ValueError(f"{who}: max_windows >= 1")
        return stride_bytes

    def _recording_logits(self, wav_data, stride_bytes, max_windows):
        """The logits of one recording's windows, in order, in pieces: on the CPU (or with an odd stride in
        bytes) one piece, ``label_batch``'s forward of ``stride(...)``; else ``label_stream``'s pieces of at
        most ``max_windows`` windows off the recording uploaded once."""
        if self.no_cuda or stride_bytes % 2:
            windows = list(stride(wav_data, stride_bytes, 2 * 16000))
            if windows:
                with torch.no_grad():
                    logits = self._net()(self._model_input(windows))
                yield logits
            return
        n = len(wav_data) // 2
        total = 0 if n < 16000 else 1 + (n - 16000) // (stride_bytes // 2)
        if total == 0:
            return
        device = next(self.model.parameters()).device
        pcm = torch.from_numpy(np.frombuffer(wav_data, dtype=np.int16, count=n).copy()).to(device)
        windows = self.audio_processor.compute_pcen_windows if self.audio_preprocess_type == "PCEN" else \
            self.audio_processor.compute_mfccs_windows
        for w0 in range(0, total, max_windows):
            with torch.no_grad():
                logits = self._net()(windows(pcm, stride_bytes // 2, 16000, w0, min(max_windows, total - w0)))
            yield logits

    def label_streams(self, recordings, stride_size_ms=500, max_windows=8192):
        """``[label_stream(r, stride_size_ms) for r in recordings]`` (int16 byte strings) with the whole
        batch in one front-end call: the bytes are concatenated and uploaded once; the recordings go, in
        order, in batches of at most ``max_windows`` windows through ``compute_mfccs_segments``
        (``compute_pcen_segments`` under PCEN), one forward, one softmax and one download per batch.  A
        recording with more than ``max_windows`` windows goes through ``label_stream`` itself.  On the
        CPU, or with an odd stride in bytes, it is ``label_stream`` per recording."""
        stride_bytes = self._stride_bytes("label_streams", stride_size_ms, max_windows)
        out = [[] for _ in recordings]
        for recs, logits, w0 in self._streams_logits(recordings, stride_bytes, max_windows):
            got = self._labelled(logits)
            for j, i in enumerate(recs):
                out[i] += got[w0[j]:w0[j + 1]]
        return out

    def _streams_logits(self, recordings, stride_bytes, max_windows):
        """``label_streams``' batching -> (recs, logits, window0) per forward: the logits of the windows of
        recordings ``recs`` (indices), recording ``recs[j]``'s rows ``window0[j]:window0[j + 1]``.  A
        recording's windows come in order; one with more than ``max_windows`` windows -- and, on the CPU or
        with an odd stride in bytes, every recording -- comes alone, in ``_recording_logits``' pieces."""
        alone = range(len(recordings))
        if not (self.no_cuda or stride_bytes % 2):
            step = stride_bytes // 2
            ns = [len(r) // 2 for r in recordings]
            Ws = [0 if n < 16000 else 1 + (n - 16000) // step for n in ns]
            alone = [i for i, w in enumerate(Ws) if w > max_windows]
        for i in alone:
            for logits in self._recording_logits(recordings[i], stride_bytes, max_windows):
                yield [i], logits, np.array([0, logits.shape[0]], np.int64)
        if self.no_cuda or stride_bytes % 2:
            return
        batched = [i for i, w in enumerate(Ws) if 0 < w <= max_windows]
        if not batched:
            return
        device = next(self.model.parameters()).device
        off = np.concatenate([[0], np.cumsum([ns[i] for i in batched])]).astype(np.int64)
        pcm = torch.from_numpy(np.concatenate([np.frombuffer(recordings[i], dtype=np.int16, count=ns[i])
                                               for i in batched])).to(device)
        segments = self.audio_processor.compute_pcen_segments if self.audio_preprocess_type == "PCEN" else \
            self.audio_processor.compute_mfccs_segments
        a = 0
        while a < len(batched):
            b, nw = a, 0
            while b < len(batched) and nw + Ws[batched[b]] <= max_windows:
                nw += Ws[batched[b]]
                b += 1
            with torch.no_grad():
                x, w0 = segments(pcm, off[a:b + 1], step, 16000)
                logits = self._net()(x)
            yield batched[a:b], logits, w0
            a = b

    def listen_streams(self, recordings, stride_size_ms=500, method="labels", keyword="command",
                       min_keyword_prob=0.85, max_windows=8192):
        """``[listen_stream(r, stride_size_ms, method, keyword, min_keyword_prob) for r in recordings]`` off
        ``label_streams``' batching -- one front-end call and one forward per batch of at most ``max_windows``
        windows -- with ``decide`` on each batch's ``window0``: every recording's answer is made from its
        ``sums`` / ``counts`` / ``hit`` (a label is a key where its count is non-zero; the early exit of
        "command_tagging" is ``hit >= 0``), no (label, prob) list is built."""
        stride_bytes = self._stride_bytes("listen_streams", stride_size_ms, max_windows)
        n_rec, n_labels = len(recordings), len(self.labels)
        sums, counts = np.zeros((n_rec, n_labels)), np.zeros((n_rec, n_labels), np.int64)
        hit, seen = np.full(n_rec, -1, np.int64), np.zeros(n_rec, np.int64)
        for recs, logits, w0 in self._streams_logits(recordings, stride_bytes, max_windows):
            _, _, s, c, h = self.decide(logits, w0, keyword, min_keyword_prob)
            recs = np.asarray(recs)
            found = (hit[recs] < 0) & (h >= 0)
            hit[recs[found]] = seen[recs[found]] + h[found]
            sums[recs] += s       # (exact: a recording's pieces add up to the sum of its windows' probs)
            counts[recs] += c
            seen[recs] += np.diff(w0)
        if method == "command_tagging":
            return [dict(contains_command=bool(h >= 0)) for h in hit]
        return [{self.labels[l]: float(sums[i, l]) for l in np.flatnonzero(counts[i])} for i in range(n_rec)]

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
    pool warns once and works as with ``device_state=False``.  ``feed_arrays`` is a bank tick fed and read
    as arrays: one int16 array in, ``(label, prob, window0)`` out."""

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
            got = svc._labelled(self._forward(x))
            for j, key in enumerate(chunks):
                out[key] = got[w0[j]:w0[j + 1]]
        return out

    def _forward(self, x):
        """The logits of a tick's windows: the forward in slices of at most MAX_WINDOWS."""
        with torch.no_grad():
            net = self.service._net()
            return torch.cat([net(x[a:a + self.MAX_WINDOWS]) for a in range(0, x.shape[0], self.MAX_WINDOWS)])

    def feed_arrays(self, keys, pcm, offsets):
        """``feed`` as arrays, for a pool on a bank (``device_state=True``; ValueError otherwise): ``pcm`` is
        one int16 numpy array or tensor holding the new samples of ``keys`` (distinct), key r's being
        ``pcm[offsets[r]:offsets[r + 1]]`` -> numpy ``(label int32 [N], prob float32 [N], window0 int64
        [len(keys) + 1])``: the windows key r completes are rows ``window0[r]:window0[r + 1]``, their label an
        index into the service's labels.  One bank tick, the forward in slices of at most MAX_WINDOWS, one
        ``decide``; apart from the key -> slot lookup nothing is done per stream.  A key is opened at its
        first feed, and may be fed through ``feed`` on another tick (whose odd-byte carry is ``feed``'s alone:
        whole samples come in here)."""
        if self.bank is None:
            raise ValueError("StreamPool.feed_arrays: the pool has no stream bank (device_state=True on a ROCm "
                             "service with an even stride in bytes)")
        if not torch.is_tensor(pcm):
            pcm = torch.from_numpy(np.ascontiguousarray(pcm))
        ids = []
        for key in keys:
            st = self._streams.get(key)
            if st is None:
                st = self._streams[key] = [self.bank.open(), b""]
            ids.append(st[0])
        x, w0 = self.bank.tick(ids, pcm, offsets)
        if not x.shape[0]:
            return np.zeros(0, np.int32), np.zeros(0, np.float32), w0
        label, prob = self.service.decide(self._forward(x))
        return label, prob, w0


def stride(array, stride_size, window_size):
    """service.py:106-110: sliding windows (server.py:104 uses 0.5 s stride, 1 s window)."""
    i = 0
    while i + window_size <= len(array):
        yield array[i:i + window_size]
        i += stride_size
