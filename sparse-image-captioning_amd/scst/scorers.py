"""SCST reward scorer — mirror of ``sparse_caption/scst/scorers.py:17-114`` (``CaptionScorer``) on top of the native,
multi-threaded host scorer of ``libortk.so`` (``include/ortk_scorer.h``): CIDEr-D (``ciderD_scorer.py``) and per-sentence
BLEU-1..4 (``bleu_scorer.py``).  Same call contract::

    scorer = CaptionScorer(path_to_cached_tokens, cider_weight=1.0, bleu_weight=None)
    sc_sample, sc_baseline = scorer(refs, sample, baseline)      # lists of lists of caption strings

``path_to_cached_tokens`` is the reference's df pickle name (``data/<name>.p`` holding ``document_frequency`` /
``ref_len``), a path to such a pickle, ``"corpus"`` / ``None`` for on-the-fly document frequencies, or a dict
``{"document_frequency": {...}, "ref_len": n}``.  :meth:`score_ids` is the fast path for token-id tensors straight from
``model(..., mode="sample")`` (no string round trip).

Device scorer: :meth:`CaptionScorer.device_refs` cooks the references of a batch into a flat pack on the host (no device
needed up to the upload: :meth:`CaptionScorer.pack_refs` runs in a data-loader worker) and :meth:`CaptionScorer.score_device`
scores the sampled token tensor in one HIP kernel on the current stream — no copy to the host, no synchronisation."""
import ctypes as C
import os
import pickle

import numpy as np

from .. import _lib as L

_P, _I32, _I64, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_SIG = {
    "ortk_scorer_create": (_P, [_I32, _D]),
    "ortk_scorer_destroy": (None, [_P]),
    "ortk_scorer_set_df": (_I32, [_P, _P, _P, _P, _I64, _D]),
    "ortk_scorer_score": (_I32, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _I32]),
    "ortk_scorer_pack_refs": (_I32, [_P, _P, _P, _P, _I64, _I32, _P, _I64, _P, _I64, _P, _P]),
    "ortk_scorer_df_table": (_I32, [_P, _P, _I64, _P]),
    "ortk_scorer_score_pack_host": (_I32, [_P]),
    "ortk_scorer_score_pack_device": (_I32, [_P, _P]),
}

BASELINE_GREEDY, BASELINE_LEAVE_ONE_OUT = 0, 1      # include/ortk_scorer.h: ORTK_SCORER_BASELINE_*
MAX_DEVICE_VOCAB = 65534                            # the kernel cannot report a token id it cannot pack: refused up front
MAX_DEVICE_ROWS, MAX_DEVICE_LEN = 64, 64            # hypothesis rows per image, tokens per row


class PackArgs(C.Structure):
    """``ortk_scorer_pack_args`` of include/ortk_scorer.h."""
    _fields_ = [("pack", _P), ("df_table", _P), ("ref_len_log", _D), ("sigma", _D), ("sample", _P), ("sample_stride", _I64),
                ("greedy", _P), ("greedy_stride", _I64), ("n", _I32), ("baseline", _I32), ("n_images", _I32), ("ns", _I32),
                ("L", _I32), ("eos", _I32), ("pad", _I32), ("reserved", _I32), ("cider_weight", _D), ("bleu_weight", _D * 4),
                ("reward", _P), ("score_sample", _P), ("score_baseline", _P)]


class RefPack:
    """The references of one batch cooked for :meth:`CaptionScorer.score_pack_host` / ``score_device``: ``pack`` and ``df``
    are uint8 arrays on the host (numpy) or tensors on the device (``df`` is the document-frequency hash table)."""

    def __init__(self, pack, df, ref_len_log, n_images, items_per_image, n, sigma, pinned=None):
        self.pack, self.df, self.ref_len_log = pack, df, float(ref_len_log)
        self.n_images, self.items_per_image, self.n, self.sigma = int(n_images), int(items_per_image), int(n), float(sigma)
        self._pinned = pinned        # the staging buffers of the asynchronous upload stay alive with the pack


def _lib():
    lib = L.lib()
    if not getattr(lib, "_scorer_bound", False):
        for name, (res, args) in _SIG.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._scorer_bound = True
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Vocab(dict):
    """word -> id interning (ids < 65535: an n-gram packs exactly into 64 bits on the native side)."""

    def ids(self, sentence):
        out = []
        for w in sentence.split():
            i = self.get(w)
            if i is None:
                i = self[w] = len(self)
                if i >= 65534:
                    raise ValueError("more than 65534 distinct words in one scorer")
            out.append(i)
        return out


class NativeScorer:
    """Thin handle on ``ortk_scorer``: captions are lists of int ids."""

    def __init__(self, n=4, sigma=6.0, nthreads=0):
        self._lib = _lib()
        self._h = self._lib.ortk_scorer_create(n, float(sigma))
        if not self._h:
            raise ValueError("bad scorer parameters")
        self.nthreads = int(nthreads)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.ortk_scorer_destroy(self._h)
            self._h = None

    def set_df(self, ngrams, counts, ref_len):
        tok = np.asarray([t for g in ngrams for t in g], dtype=np.int32)
        off = np.zeros(len(ngrams) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(g) for g in ngrams])
        df = np.asarray(counts, dtype=np.float64)
        if self._lib.ortk_scorer_set_df(self._h, _ptr(tok), _ptr(off), _ptr(df), len(ngrams), float(ref_len)) != 0:
            raise ValueError("ortk_scorer_set_df: bad n-gram table")

    def pack_refs(self, refs, items_per_image):
        """refs[i] = list of id lists (the references of image i).  Returns (pack, df_table or None, ref_len_log) as numpy
        uint8 arrays; df_table is the batch's table in corpus mode, None in cached mode (see :meth:`df_table`)."""
        caps = [c for r in refs for c in r]
        tok = np.asarray([t for c in caps for t in c], dtype=np.int64)
        if tok.size and (tok.min() < 0 or tok.max() >= 65535):
            raise ValueError("ortk_scorer_pack_refs: token id outside 0..65534")
        tok = tok.astype(np.int32)
        off = np.zeros(len(caps) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(c) for c in caps])
        roff = np.zeros(len(refs) + 1, dtype=np.int64)
        roff[1:] = np.cumsum([len(r) for r in refs])
        need = np.zeros(2, dtype=np.int64)
        rll = C.c_double(0.0)
        args = (self._h, _ptr(tok), _ptr(off), _ptr(roff), len(refs), int(items_per_image))
        rc = self._lib.ortk_scorer_pack_refs(*args, None, 0, None, 0, _ptr(need), C.byref(rll))
        if rc == 0:
            pack = np.empty(int(need[0]), dtype=np.uint8)
            df = np.empty(int(need[1]), dtype=np.uint8) if need[1] > 0 else None
            rc = self._lib.ortk_scorer_pack_refs(*args, _ptr(pack), pack.size, _ptr(df) if df is not None else None,
                                                 0 if df is None else df.size, _ptr(need), C.byref(rll))
        if rc != 0:
            raise ValueError("ortk_scorer_pack_refs: bad arguments (an image without references or a token id >= 65535)")
        return pack, df, rll.value

    def df_table(self):
        """The cached document-frequency table as the flat hash table the pack scorers read (numpy uint8)."""
        need = C.c_int64(0)
        if self._lib.ortk_scorer_df_table(self._h, None, 0, C.byref(need)) != 0:
            raise ValueError("ortk_scorer_df_table: no cached document-frequency table (corpus mode)")
        out = np.empty(need.value, dtype=np.uint8)
        if self._lib.ortk_scorer_df_table(self._h, _ptr(out), out.size, C.byref(need)) != 0:
            raise ValueError("ortk_scorer_df_table failed")
        return out

    def score(self, captions, hyp_cap, item_refs, cider=True, bleu=False):
        """captions: list of id lists; hyp_cap[i] = caption index of item i's hypothesis; item_refs[i] = list of caption
        indices of its references.  Returns (cider (n,) or None, bleu (4,n) or None)."""
        n = len(hyp_cap)
        tok = np.asarray([t for c in captions for t in c], dtype=np.int32)
        off = np.zeros(len(captions) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(c) for c in captions])
        hyp = np.asarray(hyp_cap, dtype=np.int64)
        ref = np.asarray([r for rs in item_refs for r in rs], dtype=np.int64)
        roff = np.zeros(n + 1, dtype=np.int64)
        roff[1:] = np.cumsum([len(rs) for rs in item_refs])
        c_out = np.zeros(n, dtype=np.float64) if cider else None
        b_out = np.zeros((4, n), dtype=np.float64) if bleu else None
        rc = self._lib.ortk_scorer_score(self._h, _ptr(tok), _ptr(off), len(captions), _ptr(hyp), _ptr(ref), _ptr(roff), n,
                                         _ptr(c_out) if cider else None, _ptr(b_out) if bleu else None, self.nthreads)
        if rc != 0:
            raise ValueError("ortk_scorer_score: bad arguments (empty reference list or token id >= 65535)")
        return c_out, b_out


class CaptionScorer:
    """``CaptionScorer`` of scst/scorers.py:17-107."""

    def __init__(self, path_to_cached_tokens, cider_weight=1.0, bleu_weight=None, nthreads=0):
        assert isinstance(cider_weight, float)
        if bleu_weight is None:
            bleu_weight = [0.0] * 4
        else:
            assert isinstance(bleu_weight, (list, tuple))
        assert len(bleu_weight) == 4
        self.path_to_cached_tokens = path_to_cached_tokens
        self.weights = {"ciderD": cider_weight, "bleu": list(bleu_weight)}
        self.vocab = _Vocab()
        self.native = NativeScorer(4, 6.0, nthreads)
        self._df_loaded = False
        self._df_space = None        # "words": the df table is keyed by word n-grams (the reference's pickles); "ids": by token ids
        self._df_host = None         # cached mode: the table as the flat hash table of the pack scorers (built once)
        self._df_dev = {}            # ... and its copy per device

    # ---- document frequencies (ciderD_scorer.py:82-88)
    def _load_df(self):
        if self._df_loaded:
            return
        self._df_loaded = True
        src = self.path_to_cached_tokens
        if src is None or src == "corpus":
            return
        if isinstance(src, dict):
            table = src
        else:
            path = src if os.path.isfile(src) else os.path.join("data", src + ".p")
            with open(path, "rb") as f:
                table = pickle.load(f, encoding="latin1")
        grams, counts = [], []
        kinds = set()
        for ngram, cnt in table["document_frequency"].items():
            if all(isinstance(t, (int, np.integer)) for t in ngram):     # a table cooked in token-id space: ids are used as they are
                kinds.add("ids")
                if any(int(t) < 0 or int(t) >= 65534 for t in ngram):
                    raise ValueError("token ids of a document-frequency table must be < 65534")
                grams.append([int(t) for t in ngram])
            else:                                                        # the reference's pickles: whitespace words
                kinds.add("words")
                grams.append(self.vocab.ids(" ".join(ngram)))
            counts.append(float(cnt))
        if len(kinds) > 1:
            raise ValueError("document-frequency table mixes word and token-id n-grams")
        self._df_space = kinds.pop() if kinds else None
        self.native.set_df(grams, counts, float(table["ref_len"]))

    @staticmethod
    def input_check(inputs, same_sub_len=True):
        assert isinstance(inputs, (list, tuple))
        assert all(isinstance(_, (list, tuple)) for _ in inputs)
        if same_sub_len:
            lens = set(len(_) for _ in inputs)
            assert len(lens) == 1, f"Each image should have the same number of captions. Received captions per image: {lens}"

    def __call__(self, refs, sample, baseline=None):
        self.input_check(refs, same_sub_len=False)
        self.input_check(sample)
        assert len(refs) == len(sample), f"`ref` and `sample` have different lengths: refs = {len(refs)}, sample = {len(sample)}"
        if baseline:
            self.input_check(baseline)
            assert len(sample) == len(baseline), \
                f"`sample` and `baseline` have different lengths: sample = {len(sample)}, baseline = {len(baseline)}"
        else:
            assert baseline is None, "`baseline` should be one of: None, list or tuple."
        ids = self.vocab.ids
        ref_ids = [[ids(c) for c in r] for r in refs]
        samp_ids = [[ids(c) for c in s] for s in sample]
        base_ids = [[ids(c) for c in b] for b in baseline] if baseline else None
        return self.score_ids(ref_ids, samp_ids, base_ids)

    def score_ids(self, refs, sample, baseline=None):
        """Same as ``__call__`` on lists of token-id lists: refs[i] = reference captions of image i, sample[i] = its
        sampled captions, baseline[i] = [greedy caption].  Returns ``(sc_sample (N*ns,), sc_baseline (N*ns,))``."""
        self._load_df()
        num_baseline = len(baseline) if baseline else 0
        ns = len(sample[0])
        captions, hyp_cap, item_refs = [], [], []
        ref_idx = []
        for r in refs:                       # every reference caption is cooked once, shared by the image's items
            ref_idx.append(list(range(len(captions), len(captions) + len(r))))
            captions.extend(r)
        for i in range(num_baseline):
            assert len(baseline[i]) == 1
            hyp_cap.append(len(captions)); captions.append(baseline[i][0]); item_refs.append(ref_idx[i])
        for i in range(len(sample)):
            for j in range(ns):
                hyp_cap.append(len(captions)); captions.append(sample[i][j]); item_refs.append(ref_idx[i])
        wc, wb = self.weights["ciderD"], self.weights["bleu"]
        use_c, use_b = wc > 0, max(wb) > 0
        cider, bleu = self.native.score(captions, hyp_cap, item_refs, cider=use_c, bleu=use_b)
        scores = np.zeros(len(hyp_cap), dtype=np.float64)
        if use_c:
            scores = scores + cider * wc
        if use_b:
            for k, w in enumerate(wb):
                scores = scores + bleu[k] * w
        sc_sample = scores[num_baseline:]
        if baseline:
            sc_baseline = np.repeat(scores[:num_baseline], ns)
        else:
            sums = sc_sample.reshape([-1, ns]).sum(-1)
            sc_baseline = (np.repeat(sums, ns) - sc_sample) / (ns - 1)
        return sc_sample, sc_baseline

    def score_sequences(self, refs, sample_seq, greedy_seq=None, eos_idx=3, pad_idx=0, decode=None):
        """Token tensors straight from the model: ``sample_seq`` (N, ns, L) and ``greedy_seq`` (N, 1, L) int arrays.

        The n-grams must live in the SAME space as the document-frequency table.  The reference scores decoded strings
        (utils/training.py:239-250: ``tokenizer.decode`` then whitespace words), and its df pickles are keyed by words, so:

        * ``decode`` given (a callable ``ids -> sentence``, e.g. ``tokenizer.decode``): every row is decoded and scored
          through the string path — exactly the reference's flow; ``refs[i]`` = list of reference STRINGS (``gts``);
        * no ``decode``: rows are cut at the first EOS / PAD and scored as raw token ids; ``refs[i]`` = list of id lists.
          Only valid when the document frequencies are in token-id space too — ``"corpus"`` mode or a table with integer
          n-grams; with a word-keyed table this raises instead of silently looking up unrelated n-grams."""
        s = np.asarray(sample_seq.cpu() if hasattr(sample_seq, "cpu") else sample_seq)
        g = None if greedy_seq is None else np.asarray(greedy_seq.cpu() if hasattr(greedy_seq, "cpu") else greedy_seq)
        if decode is not None:
            sample = [[decode(r) for r in img] for img in s]
            base = None if g is None else [[decode(img[0])] for img in g]
            return self(refs, sample, base)
        self._load_df()
        if self._df_space == "words":
            raise ValueError("score_sequences without `decode`: the document-frequency table is keyed by words, token ids would "
                             "look up unrelated n-grams; pass decode=tokenizer.decode (the reference's flow), use a table cooked "
                             "in token-id space, or 'corpus' document frequencies")

        def cut(row):
            out = []
            for t in row:
                t = int(t)
                if t == eos_idx or t == pad_idx:
                    break
                out.append(t)
            return out
        sample = [[cut(r) for r in img] for img in s]
        base = None if g is None else [[cut(img[0])] for img in g]
        return self.score_ids(refs, sample, base)

    # ---- reference pack: host walk and device kernel (include/ortk_scorer.h) -------------------------------------------
    def _check_id_space(self, what):
        self._load_df()
        if self._df_space == "words":
            raise ValueError(f"{what}: the document-frequency table is keyed by words, token ids would look up unrelated n-grams; "
                             "use a table cooked in token-id space or 'corpus' document frequencies (or the host path with "
                             "decode=tokenizer.decode)")

    def _cached_df(self):
        cached = self.path_to_cached_tokens is not None and self.path_to_cached_tokens != "corpus"
        if not cached:
            return None
        if self._df_host is None:
            self._df_host = self.native.df_table()
        return self._df_host

    def pack_refs(self, refs, items_per_image):
        """Cooks ``refs[i]`` (the reference id lists of image i) for a batch that scores ``items_per_image`` hypotheses per image
        (``ns``, or ``ns + 1`` with a greedy baseline; in corpus mode the document frequencies depend on it).  Host only: no
        device is needed, so a data-loader worker can run it.  Returns a :class:`RefPack` of numpy arrays."""
        self._check_id_space("pack_refs")
        self.input_check(refs, same_sub_len=False)
        pack, df, rll = self.native.pack_refs(refs, items_per_image)
        if df is None:
            df = self._cached_df()
        return RefPack(pack, df, rll, len(refs), items_per_image, 4, 6.0)

    def device_refs(self, refs, items_per_image, device, vocab_size=None):
        """:meth:`pack_refs` plus one ``non_blocking`` upload from pinned memory.  ``refs`` may be a host :class:`RefPack`
        already.  In cached mode the document-frequency table is uploaded once per scorer and device.  ``vocab_size``: the
        model's vocabulary; above 65534 the device scorer is refused (the kernel cannot report an id it cannot pack)."""
        import torch
        if vocab_size is not None and int(vocab_size) > MAX_DEVICE_VOCAB:
            raise ValueError(f"device scorer: vocab_size {vocab_size} > {MAX_DEVICE_VOCAB} (an n-gram packs four 16-bit ids)")
        hp = refs if isinstance(refs, RefPack) else self.pack_refs(refs, items_per_image)
        if hp.items_per_image != int(items_per_image):
            raise ValueError("device_refs: the pack was cooked for another items_per_image")
        device = torch.device(device)
        pinned = []

        def up(a):
            t = torch.from_numpy(a).pin_memory()
            pinned.append(t)
            return t.to(device, non_blocking=True)
        cached = hp.df is not None and hp.df is self._df_host
        if cached:
            key = str(device)
            if key not in self._df_dev:
                self._df_dev[key] = up(hp.df)
            df = self._df_dev[key]
        else:
            df = None if hp.df is None else up(hp.df)
        return RefPack(up(hp.pack), df, hp.ref_len_log, hp.n_images, hp.items_per_image, hp.n, hp.sigma, pinned=pinned)

    def _pack_args(self, rp, n_images, ns, L, has_greedy, eos_idx, pad_idx):
        if n_images != rp.n_images:
            raise ValueError(f"the pack holds {rp.n_images} images, the token tensor {n_images}")
        if ns + has_greedy != rp.items_per_image:
            raise ValueError(f"the pack was cooked for {rp.items_per_image} hypotheses per image, the call scores {ns + has_greedy}")
        if not has_greedy and ns < 2:
            raise ValueError("the leave-one-out baseline needs at least two samples per image")
        if ns + has_greedy > MAX_DEVICE_ROWS or not 1 <= L <= MAX_DEVICE_LEN:
            raise ValueError(f"pack scorer: at most {MAX_DEVICE_ROWS} rows per image of at most {MAX_DEVICE_LEN} tokens")
        a = PackArgs()
        a.ref_len_log, a.sigma, a.n = rp.ref_len_log, rp.sigma, rp.n
        a.baseline = BASELINE_GREEDY if has_greedy else BASELINE_LEAVE_ONE_OUT
        a.n_images, a.ns, a.L, a.eos, a.pad = n_images, ns, L, int(eos_idx), int(pad_idx)
        a.cider_weight = self.weights["ciderD"]
        a.bleu_weight = (_D * 4)(*self.weights["bleu"])
        return a

    def score_pack_host(self, ref_pack, sample_seq, greedy_seq=None, eos_idx=3, pad_idx=0):
        """The host walk of a pack (the scoring core the kernel runs, on the CPU): ``sample_seq`` (N, ns, L) and ``greedy_seq``
        (N, 1, L) integer arrays.  Returns ``(reward fp32, sc_sample, sc_baseline)`` numpy arrays of N * ns entries."""
        s = np.ascontiguousarray(np.asarray(sample_seq), dtype=np.int64)
        g = None if greedy_seq is None else np.ascontiguousarray(np.asarray(greedy_seq), dtype=np.int64)
        N, ns, L = s.shape
        a = self._pack_args(ref_pack, N, ns, L, g is not None, eos_idx, pad_idx)
        reward, scs, scb = np.zeros(N * ns, np.float32), np.zeros(N * ns, np.float64), np.zeros(N * ns, np.float64)
        a.pack, a.df_table = _ptr(ref_pack.pack), None if ref_pack.df is None else _ptr(ref_pack.df)
        a.sample, a.sample_stride = _ptr(s), L
        if g is not None:
            assert g.shape == (N, 1, L), g.shape
            a.greedy, a.greedy_stride = _ptr(g), L
        a.reward, a.score_sample, a.score_baseline = _ptr(reward), _ptr(scs), _ptr(scb)
        if _lib().ortk_scorer_score_pack_host(C.byref(a)) != 0:
            raise ValueError("ortk_scorer_score_pack_host: bad arguments (token id outside 0..65534, or not a pack of this batch)")
        return reward, scs, scb

    def score_device(self, device_refs, sample_seq, greedy_seq=None, eos_idx=3, pad_idx=0):
        """One HIP kernel on the current stream: ``sample_seq`` (N, ns, L) and ``greedy_seq`` (N, 1, L) int64 device tensors as
        the decode left them -> ``(reward fp32 (N*ns,), sc_sample, sc_baseline fp64 (N*ns,))`` device tensors.  Greedy baseline
        when ``greedy_seq`` is given, leave-one-out otherwise.  No host synchronisation.  Raw token ids: the same rule as
        :meth:`score_sequences` without ``decode`` (a word-keyed table is refused when the pack is cooked)."""
        import torch
        rp = device_refs
        if not (isinstance(rp, RefPack) and torch.is_tensor(rp.pack) and rp.pack.is_cuda):
            raise ValueError("score_device needs the result of device_refs()")
        if not (sample_seq.is_cuda and sample_seq.dtype == torch.int64 and sample_seq.dim() == 3):
            raise ValueError("score_device: sample_seq must be an int64 device tensor (N, ns, L)")
        N, ns, T = sample_seq.shape
        s = sample_seq if sample_seq.is_contiguous() else sample_seq.contiguous()
        a = self._pack_args(rp, N, ns, T, greedy_seq is not None, eos_idx, pad_idx)
        a.pack, a.df_table = _dptr(rp.pack), _dptr(rp.df)
        a.sample, a.sample_stride = _dptr(s), T
        g = None
        if greedy_seq is not None:
            if not (greedy_seq.is_cuda and greedy_seq.dtype == torch.int64 and tuple(greedy_seq.shape) == (N, 1, T)):
                raise ValueError("score_device: greedy_seq must be an int64 device tensor (N, 1, L)")
            g = greedy_seq if greedy_seq.is_contiguous() else greedy_seq.contiguous()
            a.greedy, a.greedy_stride = _dptr(g), T
        reward = torch.empty(N * ns, dtype=torch.float32, device=s.device)
        sc = torch.empty(2, N * ns, dtype=torch.float64, device=s.device)
        a.reward, a.score_sample, a.score_baseline = _dptr(reward), _dptr(sc[0]), _dptr(sc[1])
        with torch.cuda.device(s.device):
            L.check(_lib().ortk_scorer_score_pack_device(C.byref(a), L.stream_ptr()), "ortk_scorer_score_pack_device")
        return reward, sc[0], sc[1]


def _dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
