"""CTCLoss -- host-side mirror of the reference's ``src/wav2vec2/losses.py:4-56``.

Same constructor ``CTCLoss(config, model_input_shape, division_factor=1)`` and
call ``loss(labels, logits) -> scalar``; the reference's conventions are kept:
  * every row's ``logit_length`` is the FULL frame count derived from the static
    ``model_input_shape`` (not from real audio length) -- losses.py:29-30,47-56;
  * ``label_length`` = number of labels != ``pad_id`` -- losses.py:32-33;
  * blank index = ``pad_id``; per-sample NLL / ``division_factor``, then
    Keras ``Reduction.SUM`` -- losses.py:6,45.
The alpha/beta recursions run in the HIP library (w2v2_ctc_loss).

``expected_risk`` and ``MWERLoss`` are sequence-level losses over n-best lists: the expected number of errors under
the list's renormalised exact CTC posteriors, with its gradient from w2v2_ctc_score_grad.  They have no counterpart in the reference.

``StarCTCLoss`` and ``star_labels`` are the CTC loss for partial transcripts: label rows may hold the star, the
wildcard label of ``alignment.forced_align``; the loss and its gradient come from w2v2_ctc_score_grad_star.
"""

import math

import numpy as np

from . import _native as N


class CTCLoss:
    def __init__(self, config, model_input_shape, division_factor=1):
        self.kernal_sizes = config.kernal_sizes
        self.strides = config.strides
        self.pad_id = config.pad_id
        self.division_factor = division_factor
        self.model_input_shape = model_input_shape

    def _get_logit_length(self, input_length):
        """Frames at the end of the conv stack (losses.py:47-56)."""
        for kernal_size, stride in zip(self.kernal_sizes, self.strides):
            input_length = 1 + (input_length - kernal_size) // stride
        return input_length

    def per_sample(self, labels, logits, with_grad=False, with_total=False):
        """Per-sample NLL (B,) [and d sum(nll) / d logits] [and the scalar the reference's `call` returns: sum_b nll_b / division_factor];
        torch CUDA tensors."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("CTCLoss (MI355X build) needs a HIP device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        if not isinstance(logits, torch.Tensor):
            logits = torch.as_tensor(np.asarray(logits, dtype=np.float32))
        logits = logits.detach().as_subclass(torch.Tensor).to(device=dev, dtype=torch.float32).contiguous()
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
            # host labels: a label outside the vocabulary is a vocab / config mismatch -- say so before the launch.
            # (Device-resident labels are checked by the kernel instead: the sample's loss comes back NaN.)
            host = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
            if host.size and (host.min() < 0 or host.max() >= logits.shape[-1]):
                raise ValueError(f"labels must lie in [0, {logits.shape[-1]}): got [{host.min()}, {host.max()}]")
            labels = torch.as_tensor(host)
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
        B, T, V = logits.shape
        if labels.dim() != 2 or labels.shape[0] != B:
            raise ValueError("labels must be (batch, max_label_len)")
        U = labels.shape[1]
        logit_len = int(self._get_logit_length(int(self.model_input_shape[1])))
        if logit_len > T:
            raise ValueError(f"model_input_shape implies {logit_len} frames but logits have {T}")
        nll = torch.empty((B,), device=dev, dtype=torch.float32)
        grad = torch.empty_like(logits) if with_grad else None
        total = torch.empty((1,), device=dev, dtype=torch.float32)
        lib = N.load()
        # label lengths (count of labels != pad_id), the uniform logit length, the division of loss and gradient by division_factor and
        # the SUM reduction are all evaluated by the native call: no framework kernel runs between the forward and the backward
        N.check(lib.w2v2_ctc_loss_fused(N.ptr(logits), B, T, V, N.ptr(labels), U, logit_len, self.pad_id, float(self.division_factor),
                                        N.ptr(nll), N.ptr(grad), N.ptr(total), N.current_stream()), "w2v2_ctc_loss_fused")
        self.last_total = total[0]            # sum_b nll_b / division_factor, a 0-d device tensor view (kept for callers that read the
                                              # attribute; `total()` and `__call__` do not depend on it: two interleaved calls stay correct)
        if with_total:
            return (nll, grad, total[0]) if with_grad else (nll, total[0])
        if with_grad:
            return nll, grad                  # grad already / division_factor
        return nll

    def __call__(self, labels, hidden_states):
        return self.per_sample(labels, hidden_states, with_total=True)[1]

    call = __call__


def _expected_risk(logits, lists, risks, blank, frame_lengths, posterior_scale, prior, ctc, ctc_weight, max_workspace_bytes=8 << 30):
    """``expected_risk`` and what it used: (L, grad, posteriors per utterance, logp per utterance)"""
    from . import decoding as D
    lists = [[tuple(int(v) for v in h) for h in hyps] for hyps in lists]
    n = len(lists)
    have = int(logits.shape[0]) if hasattr(logits, "shape") else len(logits)
    if n != have:
        raise ValueError(f"{n} lists for {have} utterances")
    scale = float(posterior_scale)
    weight = float(ctc_weight)
    if not (scale >= 0.0 and math.isfinite(scale)):
        raise ValueError(f"posterior_scale {posterior_scale} must be finite and non-negative")
    if not (weight >= 0.0 and math.isfinite(weight)):
        raise ValueError(f"ctc_weight {ctc_weight} must be finite and non-negative")
    risks = [np.asarray(list(r), dtype=np.float64).reshape(-1) for r in risks]
    if len(risks) != n:
        raise ValueError(f"{len(risks)} rows of risks for {n} lists")
    if prior is None:
        prior = [np.zeros(len(h)) for h in lists]
    else:
        prior = [np.asarray(list(p), dtype=np.float64).reshape(-1) for p in prior]
        if len(prior) != n:
            raise ValueError(f"{len(prior)} rows of priors for {n} lists")
    for i, hyps in enumerate(lists):
        if len(set(hyps)) != len(hyps):
            raise ValueError(f"utterance {i}: the list holds a hypothesis twice; posteriors are over distinct label sequences")
        if risks[i].size != len(hyps) or prior[i].size != len(hyps):
            raise ValueError(f"utterance {i}: {len(hyps)} hypotheses with {risks[i].size} risks and {prior[i].size} priors")
        if hyps and not ((risks[i] >= 0).all() and np.isfinite(risks[i]).all()):
            raise ValueError(f"utterance {i}: risks must be finite and non-negative")
        if hyps and not np.isfinite(prior[i]).all():
            raise ValueError(f"utterance {i}: priors must be finite")
    refs = None
    if ctc is not None:
        refs = [tuple(int(v) for v in r) for r in ctc]
        if len(refs) != n:
            raise ValueError(f"{len(refs)} references for {n} lists")
    flat = [h for hyps in lists for h in hyps]
    utt = [i for i, hyps in enumerate(lists) for _ in hyps]
    if not flat and refs is None:
        raise ValueError("no hypothesis in any list and no `ctc` reference: nothing to differentiate")
    L = np.zeros(n)
    post = [np.zeros(len(hyps)) for hyps in lists]
    coef = np.zeros(len(flat))
    logp = np.zeros(0)
    if flat:
        logp = np.asarray(D.ctc_score(logits, [list(h) for h in flat], blank=blank, frame_lengths=frame_lengths, utterance=utt), np.float64)
        at = 0
        for i, hyps in enumerate(lists):
            k = len(hyps)
            lp = logp[at:at + k]
            ok = np.isfinite(lp)
            if ok.any():
                z = scale * lp[ok] + prior[i][ok]
                e = np.exp(z - z.max())
                P = e / e.sum()
                L[i] = float((P * risks[i][ok]).sum())
                post[i][ok] = P
                coef[at:at + k][ok] = scale * P * (risks[i][ok] - L[i])
            at += k
    labels, coefs, utts = [list(h) for h in flat], coef, list(utt)
    if refs is not None:
        labels += [list(r) for r in refs]
        coefs = np.concatenate((coef, np.full(n, -weight)))
        utts += list(range(n))
    logp_all, grad = D.ctc_score_grad(logits, labels, coefs, blank=blank, frame_lengths=frame_lengths, utterance=utts,
                                      max_workspace_bytes=max_workspace_bytes)
    logp_all = np.asarray(logp_all, np.float64)
    if refs is not None and weight != 0.0:
        L = L - weight * logp_all[len(flat):]
    at, per_utt = 0, []
    for hyps in lists:
        per_utt.append(logp_all[at:at + len(hyps)].copy())
        at += len(hyps)
    return L, grad, post, per_utt


def expected_risk(logits, lists, risks, blank=0, frame_lengths=None, posterior_scale=1.0, prior=None, ctc=None, ctc_weight=0.0):
    """The expected risk of given n-best lists under their renormalised exact CTC posteriors, with its gradient: model-free.

    ``logits``: what ``decoding.ctc_score`` accepts.  ``lists[i]``: the id sequences of utterance i (none twice: ValueError);
    ``risks[i][j]``: any non-negative number, such as the word errors of hypothesis j; ``prior[i][j]``: an optional additive
    log-score, such as a hypothesis' language-model part.  With ``logp_j`` the exact CTC log-probability,
    ``P_j = softmax_j(posterior_scale * logp_j + prior_j)`` over the hypotheses of the list whose ``logp`` is finite,
    ``L_i = sum_j P_j risk_j``, and the gradient is ``sum_j c_j d logp_j / d logits`` with ``c_j = posterior_scale * P_j (risk_j - L_i)``.
    An utterance without a hypothesis of finite ``logp`` has ``L_i = 0`` and no gradient from its list.  ``ctc``: one reference id
    sequence per utterance; it adds ``-ctc_weight * logp_ref`` to ``L_i`` through one more pair with ``c = -ctc_weight`` in the same
    gradient call.  Returns ``(L, grad)``: ``L`` a float64 numpy array per utterance, ``grad`` = d sum_i L_i / d logits in the
    form of ``logits`` (``decoding.ctc_score_grad``).  One ``ctc_score`` call for the posteriors and one ``ctc_score_grad`` call:
    the alpha sweep runs twice (profiles/mwer.md prices it)."""
    L, grad, _, _ = _expected_risk(logits, lists, risks, int(blank), frame_lengths, posterior_scale, prior, ctc, ctc_weight)
    return L, grad


def split_at(ids, delimiter_id):
    """The words of an id sequence: the runs between delimiters, as tuples; empty runs dropped."""
    words, cur = [], []
    for v in ids:
        if v == delimiter_id:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(int(v))
    if cur:
        words.append(tuple(cur))
    return words


def build_lists(hypotheses, references, include_reference=True, with_prior=False):
    """The lists ``MWERLoss`` trains on: per utterance the distinct id sequences of ``hypotheses[i]`` (``decoding.Hypothesis``; a
    repeated one keeps its first entry), their priors (``total - score`` when ``with_prior``, else 0), and -- with
    ``include_reference`` -- the reference appended with prior 0 unless a hypothesis already equals it.  Returns (lists, priors)."""
    lists, priors = [], []
    for hyps, ref in zip(hypotheses, references):
        ids, pr = [], []
        for h in hyps:
            t = tuple(int(v) for v in h.ids)
            if t in ids:
                continue
            ids.append(t)
            lm = h.total - h.score if with_prior else 0.0
            pr.append(lm if math.isfinite(lm) else 0.0)
        ref = tuple(int(v) for v in ref)
        if include_reference and ref not in ids:
            ids.append(ref)
            pr.append(0.0)
        lists.append(ids)
        priors.append(pr)
    return lists, priors


def token_pool(lists, references, unit, delimiter_id):
    """(pool, pairs) for ``metrics.edit_distance_pairs``: every hypothesis and reference as the tokens of ``unit`` -- "char": the ids
    themselves; "word": the id sequence split at ``delimiter_id`` and each word interned to an integer (one table for the call) --
    and one (hypothesis, reference) index pair per hypothesis, in list order."""
    table = {}

    def tokens(ids):
        if unit == "char":
            return np.asarray(ids, np.int32).reshape(-1)
        return np.asarray([table.setdefault(w, len(table)) for w in split_at(ids, delimiter_id)], np.int32).reshape(-1)

    pool, pairs = [], []
    for hyps, ref in zip(lists, references):
        r = len(pool)
        pool.append(tokens(ref))
        for h in hyps:
            pairs.append((len(pool), r))
            pool.append(tokens(h))
    return pool, pairs


class MWERLoss:
    """Minimum word error rate training: per utterance the expected number of word (or character) errors over the n best
    hypotheses of a beam search on the step's own logits, under their renormalised exact CTC posteriors (``expected_risk``).

    ``CTCLoss``'s constructor arguments and calling protocol -- ``per_sample(labels, logits, with_grad=False, with_total=False)`` and
    ``__call__`` --, so ``Trainer(model, MWERLoss(...))`` works as it stands.  Frame lengths follow ``CTCLoss``'s convention (the
    full frame count from ``model_input_shape``) unless ``per_sample`` is given ``frame_lengths=``; references are the label rows
    without ``pad_id``, which is the blank.  ``beam_width``, ``nbest``, ``lm``, ``bias``: ``decoding.beam_search``'s; with an ``lm``
    each hypothesis' ``total - score`` is its prior.  ``include_reference``: the reference joins the list (prior 0) unless a
    hypothesis already equals it.  ``unit``: "word" (ids split at ``delimiter_id``, words interned) or "char".  ``ctc_weight``
    interpolates the CTC loss of the reference, ``L_i - ctc_weight * logp_ref``, from the same gradient call; 0.01 is the
    interpolation convention of the MWER literature, NOT a value tuned on this model.  The gradient and the total are divided by
    ``division_factor``.  ``last_lists``, ``last_risks`` and ``last_posteriors`` keep what the last call used."""

    def __init__(self, config, model_input_shape, division_factor=1, beam_width=8, nbest=4, unit="word", delimiter_id=None,
                 include_reference=True, ctc_weight=0.01, posterior_scale=1.0, lm=None, bias=None):
        self._ctc = CTCLoss(config, model_input_shape, division_factor)
        self.pad_id = config.pad_id
        self.vocab_size = getattr(config, "vocab_size", None)
        self.division_factor = division_factor
        self.model_input_shape = model_input_shape
        if not float(division_factor) > 0:
            raise ValueError(f"division_factor {division_factor} must be positive")
        if int(beam_width) < 1 or int(nbest) < 1 or int(nbest) > int(beam_width):
            raise ValueError(f"need 1 <= nbest <= beam_width, got nbest {nbest}, beam_width {beam_width}")
        if unit not in ("word", "char"):
            raise ValueError(f"unit must be 'word' or 'char', got {unit!r}")
        if unit == "word":
            if delimiter_id is None:
                raise ValueError("unit='word' needs `delimiter_id`, the id that separates words")
            if int(delimiter_id) == int(config.pad_id):
                raise ValueError(f"delimiter_id {delimiter_id} is the blank (pad_id)")
            if self.vocab_size is not None and not 0 <= int(delimiter_id) < int(self.vocab_size):
                raise ValueError(f"delimiter_id {delimiter_id} outside the vocabulary [0, {self.vocab_size})")
        if not (float(ctc_weight) >= 0.0 and math.isfinite(float(ctc_weight))):
            raise ValueError(f"ctc_weight {ctc_weight} must be finite and non-negative")
        if not (float(posterior_scale) >= 0.0 and math.isfinite(float(posterior_scale))):
            raise ValueError(f"posterior_scale {posterior_scale} must be finite and non-negative")
        self.beam_width, self.nbest = int(beam_width), int(nbest)
        self.unit = unit
        self.delimiter_id = None if delimiter_id is None else int(delimiter_id)
        self.include_reference = bool(include_reference)
        self.ctc_weight, self.posterior_scale = float(ctc_weight), float(posterior_scale)
        self.lm, self.bias = lm, bias
        self.last_lists = self.last_risks = self.last_posteriors = None

    def per_sample(self, labels, logits, with_grad=False, with_total=False, frame_lengths=None):
        """Per-sample loss (B,) [and d sum(loss) / d logits / division_factor] [and sum_b loss_b / division_factor]; torch CUDA
        tensors, as ``CTCLoss.per_sample``."""
        import torch
        from . import decoding as D
        from . import metrics as M
        if not torch.cuda.is_available():
            raise RuntimeError("MWERLoss (MI355X build) needs a HIP device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        if not isinstance(logits, torch.Tensor):
            logits = torch.as_tensor(np.asarray(logits, dtype=np.float32))
        logits = logits.detach().as_subclass(torch.Tensor).to(device=dev, dtype=torch.float32).contiguous()
        if logits.dim() != 3:
            raise ValueError("logits must be (batch, frames, vocabulary)")
        B, T, V = logits.shape
        host = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
        if host.ndim != 2 or host.shape[0] != B:
            raise ValueError("labels must be (batch, max_label_len)")
        if host.size and (host.min() < 0 or host.max() >= V):
            raise ValueError(f"labels must lie in [0, {V}): got [{host.min()}, {host.max()}]")
        if frame_lengths is None:
            logit_len = int(self._ctc._get_logit_length(int(self.model_input_shape[1])))
            if logit_len > T:
                raise ValueError(f"model_input_shape implies {logit_len} frames but logits have {T}")
            frame_lengths = [logit_len] * B
        frame_lengths = [int(v) for v in frame_lengths]
        refs = [tuple(int(v) for v in row if v != self.pad_id) for row in host]
        hyps = D.beam_search(logits, beam_width=self.beam_width, nbest=self.nbest, blank=self.pad_id, frame_lengths=frame_lengths,
                             lm=self.lm, bias=self.bias)
        lists, priors = build_lists(hyps, refs, self.include_reference, with_prior=self.lm is not None)
        pool, pairs = token_pool(lists, refs, self.unit, self.delimiter_id)
        counts = M.edit_distance_pairs(pool, pairs)
        risks, at = [], 0
        for h in lists:
            risks.append([float(c[0]) for c in counts[at:at + len(h)]])
            at += len(h)
        ctc = refs if self.ctc_weight != 0.0 else None
        if ctc is None and not any(lists):
            L, grad, post = np.zeros(B), torch.zeros_like(logits), [np.zeros(0) for _ in lists]
        else:
            L, grad, post, _ = _expected_risk(logits, lists, risks, self.pad_id, frame_lengths, self.posterior_scale, priors, ctc,
                                              self.ctc_weight)
        self.last_lists, self.last_risks, self.last_posteriors = lists, risks, post
        loss = torch.from_numpy(L.astype(np.float32)).to(dev)
        total = torch.from_numpy(np.asarray(L.sum() / float(self.division_factor), np.float32).reshape(1)).to(dev)
        self.last_total = total[0]
        if with_grad and float(self.division_factor) != 1.0:
            grad = grad / float(self.division_factor)
        if with_total:
            return (loss, grad, total[0]) if with_grad else (loss, total[0])
        if with_grad:
            return loss, grad
        return loss

    def __call__(self, labels, hidden_states):
        return self.per_sample(labels, hidden_states, with_total=True)[1]

    call = __call__


def star_labels(texts, tokenizer, star="*", free_ends=False, vocab_size=None, pad_id=None):
    """The label rows ``StarCTCLoss`` trains on, from partial transcripts: each text is encoded with ``tokenizer`` through
    ``alignment.star_transcript`` -- a whitespace-separated word equal to ``star`` becomes the star label V and the word delimiter
    next to it is dropped; ``free_ends`` puts a star before the first and after the last label; a sequence of ids is used as it is
    and may hold V -- and the rows are padded to one length with ``pad_id``.  V is ``vocab_size`` (default: ``len(tokenizer
    .get_vocab())``) and ``pad_id`` defaults to the tokenizer's "<pad>", the blank.  Returns an int32 numpy array (batch, max
    length); a row with two stars next to each other raises ValueError."""
    from .alignment import star_transcript
    if isinstance(texts, str):
        raise ValueError("`texts` is a list of transcripts, one per utterance")
    vocab = tokenizer.get_vocab() if tokenizer is not None and hasattr(tokenizer, "get_vocab") else None
    if vocab_size is None:
        if vocab is None:
            raise ValueError("without a tokenizer that has get_vocab(): pass vocab_size, the star's id")
        vocab_size = len(vocab)
    if pad_id is None:
        if vocab is None or "<pad>" not in vocab:
            raise ValueError("the tokenizer names no '<pad>': pass pad_id, the blank")
        pad_id = vocab["<pad>"]
    V, pad_id = int(vocab_size), int(pad_id)
    rows = []
    for i, tr in enumerate(texts):
        ids = star_transcript(tr, V, tokenizer, star, free_ends)
        if any(a == V and b == V for a, b in zip(ids, ids[1:])):
            raise ValueError(f"transcript {i}: two stars next to each other; collapse them into one")
        if any(v == pad_id for v in ids):
            raise ValueError(f"transcript {i}: label {pad_id} is the padding (the blank)")
        rows.append(ids)
    width = max([len(r) for r in rows] + [1])
    out = np.full((len(rows), width), pad_id, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


class StarCTCLoss:
    """The CTC loss for partial transcripts: ``nll_b = -logp_b`` with ``logp_b`` the exact star score of
    ``decoding.ctc_score(..., star_score=star_score)``, in fp64 log space, for any frame counts and up to 8191 labels.

    ``CTCLoss``'s constructor arguments and calling protocol -- ``per_sample(labels, logits, with_grad=False, with_total=False)``
    and ``__call__`` --, so ``Trainer(model, StarCTCLoss(...))`` works as it stands.  Label rows are padded with ``pad_id`` (the
    blank) and may hold the star's id V = ``logits.shape[-1]`` (``star_labels`` builds them from text).  Frame lengths follow
    ``CTCLoss``'s convention (the full frame count from ``model_input_shape``) unless ``per_sample`` is given ``frame_lengths=``.
    The gradient comes from ONE ``decoding.ctc_score_grad`` call with ``coef = -1 / division_factor``; the total is
    ``sum_b nll_b / division_factor``.  A sample whose labels its frames cannot hold has ``nll = inf`` and no gradient.

    What the loss does on star frames: in proportion to the star's occupancy it sharpens the model's own top token; it does not
    supervise which token.  With a star ``nll`` may be negative: the star's column is not part of the softmax.
    ``star_score = -0.5`` is the aligner's convention, not a value tuned here."""

    def __init__(self, config, model_input_shape, division_factor=1, star_score=-0.5):
        from .alignment import _check_star_score
        self._ctc = CTCLoss(config, model_input_shape, division_factor)
        self.pad_id = config.pad_id
        self.division_factor = division_factor
        self.model_input_shape = model_input_shape
        if not float(division_factor) > 0:
            raise ValueError(f"division_factor {division_factor} must be positive")
        self.star_score = _check_star_score(star_score)

    def per_sample(self, labels, logits, with_grad=False, with_total=False, frame_lengths=None):
        """Per-sample loss (B,) [and d sum(loss) / d logits / division_factor] [and sum_b loss_b / division_factor]; torch CUDA
        tensors, as ``CTCLoss.per_sample``."""
        import torch
        from . import decoding as D
        if not torch.cuda.is_available():
            raise RuntimeError("StarCTCLoss (MI355X build) needs a HIP device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        if not isinstance(logits, torch.Tensor):
            logits = torch.as_tensor(np.asarray(logits, dtype=np.float32))
        logits = logits.detach().as_subclass(torch.Tensor).to(device=dev, dtype=torch.float32).contiguous()
        if logits.dim() != 3:
            raise ValueError("logits must be (batch, frames, vocabulary)")
        B, T, V = logits.shape
        host = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
        if host.ndim != 2 or host.shape[0] != B:
            raise ValueError("labels must be (batch, max_label_len)")
        if host.size and (host.min() < 0 or host.max() > V):
            raise ValueError(f"labels must lie in [0, {V}] ({V} is the star): got [{host.min()}, {host.max()}]")
        if frame_lengths is None:
            logit_len = int(self._ctc._get_logit_length(int(self.model_input_shape[1])))
            if logit_len > T:
                raise ValueError(f"model_input_shape implies {logit_len} frames but logits have {T}")
            frame_lengths = [logit_len] * B
        frame_lengths = [int(v) for v in frame_lengths]
        rows = [[int(v) for v in row if v != self.pad_id] for row in host]
        div = float(self.division_factor)
        if with_grad:
            logp, grad = D.ctc_score_grad(logits, rows, [-1.0 / div] * B, blank=self.pad_id, frame_lengths=frame_lengths,
                                          star_score=self.star_score)
        else:
            logp, grad = D.ctc_score(logits, rows, blank=self.pad_id, frame_lengths=frame_lengths, star_score=self.star_score), None
        nll = -np.asarray(logp, np.float64)
        loss = torch.from_numpy(nll.astype(np.float32)).to(dev)
        total = torch.from_numpy(np.asarray(nll.sum() / div, np.float32).reshape(1)).to(dev)
        self.last_total = total[0]
        if with_total:
            return (loss, grad, total[0]) if with_grad else (loss, total[0])
        if with_grad:
            return loss, grad
        return loss

    def __call__(self, labels, hidden_states):
        return self.per_sample(labels, hidden_states, with_total=True)[1]

    call = __call__
