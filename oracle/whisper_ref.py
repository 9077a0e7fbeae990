"""ORACLE (test infrastructure, NOT product code) — CPU restatement of the Whisper
encoder-decoder forward and of HuggingFace's greedy / beam-search decoding, in plain
torch fp32 on the host.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.

The reference's arithmetic for this part of the path lives in a THIRD-PARTY dependency
that is not under /root/reference: `transformers` (pinned 4.38.2 in the reference's
requirements.txt:1; 5.15.0 is what is installed in the image).  Call sites in the
reference: model.py:609-619 and model.py:655-666 (`model.generate(...)`).  What is
restated here, citing the installed HF sources:

  encoder_forward     HF models/whisper/modeling_whisper.py:592-646 (encoder), :360-413 (layer),
                      :241-357 (attention; q scaled by head_dim**-0.5, k_proj has no bias)
  Decoder.step        HF modeling_whisper.py:690-796 (decoder), :416-506 (layer), :970,1080 (tied proj_out)
  generate (beams>1)  HF generation/utils.py:3208-3510 (_beam_search) + helpers :3008-3206
  generate (beams==1) HF generation/utils.py `_sample` with do_sample False (the reference passes
                      do_sample=True, top_k=1 which is the deterministic argmax, model.py:615-616)
  logits processors   HF generation/logits_process.py: SuppressTokensAtBeginLogitsProcessor (:1816),
                      SuppressTokensLogitsProcessor (:1869), wired by generation_whisper.py:1774-1812

Pinning: tests/test_oracle_model.py checks this file against tests/golden/tiny_*.npz —
encoder outputs, first-step logits and token sequences captured from HF `generate` driven
through the reference's own WhisperSegmenterForEval (tools/make_golden.py).
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F


@dataclass
class RefConfig:
    d_model: int
    encoder_layers: int
    decoder_layers: int
    heads: int
    ffn: int
    vocab_size: int
    n_mels: int = 80
    max_source_positions: int = 500
    max_target_positions: int = 448

    @staticmethod
    def from_hf_dict(c):
        return RefConfig(
            d_model=c["d_model"], encoder_layers=c["encoder_layers"], decoder_layers=c["decoder_layers"],
            heads=c["encoder_attention_heads"], ffn=c["encoder_ffn_dim"], vocab_size=c["vocab_size"],
            n_mels=c.get("num_mel_bins", 80), max_source_positions=c.get("max_source_positions", 500),
            max_target_positions=c.get("max_target_positions", 448))


@dataclass
class GenParams:
    prompt: list
    eos_token_id: int
    pad_token_id: int
    max_length: int = 448
    num_beams: int = 4
    length_penalty: float = 1.0
    suppress_tokens: list = field(default_factory=list)
    begin_suppress_tokens: list = field(default_factory=list)
    top_k: int = 1                      # num_beams == 1: > 1 samples among the top_k processed logits
    top_p: float = 1.0
    seed: int = 0
    window_max_length: list = None      # per-window caps on the total length (clamped to [len(prompt) + 1, max_length])


def _lin(x, sd, prefix, bias=True):
    return F.linear(x, sd[prefix + ".weight"], sd[prefix + ".bias"] if bias else None)


def _ln(x, sd, prefix):
    return F.layer_norm(x, (x.shape[-1],), sd[prefix + ".weight"], sd[prefix + ".bias"], 1e-5)


def _heads(x, h):
    b, t, d = x.shape
    return x.view(b, t, h, d // h).transpose(1, 2)


def _attn(q, k, v, mask=None):
    """q already scaled.  q [B,H,Tq,64], k/v [B,H,Tk,64]."""
    w = torch.matmul(q, k.transpose(-1, -2))
    if mask is not None:
        w = w + mask
    w = torch.softmax(w, dim=-1)
    o = torch.matmul(w, v)
    b, h, t, e = o.shape
    return o.transpose(1, 2).reshape(b, t, h * e)


@torch.no_grad()
def encoder_forward(sd, cfg, feats, return_hidden=False):
    """feats float32 [B,80,1000] -> [B,500,d]."""
    p = "model.encoder."
    x = F.gelu(F.conv1d(feats, sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"], stride=2, padding=1))
    x = x.permute(0, 2, 1) + sd[p + "embed_positions.weight"][None, : x.shape[-1]]
    scale = (cfg.d_model // cfg.heads) ** -0.5
    hidden = [x]
    for i in range(cfg.encoder_layers):
        lp = f"{p}layers.{i}."
        r = x
        y = _ln(x, sd, lp + "self_attn_layer_norm")
        q = _heads(_lin(y, sd, lp + "self_attn.q_proj") * scale, cfg.heads)
        k = _heads(_lin(y, sd, lp + "self_attn.k_proj", bias=False), cfg.heads)
        v = _heads(_lin(y, sd, lp + "self_attn.v_proj"), cfg.heads)
        x = r + _lin(_attn(q, k, v), sd, lp + "self_attn.out_proj")
        r = x
        y = _ln(x, sd, lp + "final_layer_norm")
        y = F.gelu(_lin(y, sd, lp + "fc1"))
        x = r + _lin(y, sd, lp + "fc2")
        hidden.append(x)
    x = _ln(x, sd, p + "layer_norm")
    return (x, hidden) if return_hidden else x


class Decoder:
    """Incremental decoder with self-attention KV cache; cross K/V computed once per row."""

    def __init__(self, sd, cfg, enc_out, keep_dtype=False):
        """keep_dtype: step() returns the logits in the dtype of `sd` / `enc_out` (float64 weights and encoder output: a float64
        reference) instead of casting them to fp32."""
        self.sd, self.cfg, self.keep_dtype = sd, cfg, keep_dtype
        self.p = "model.decoder."
        self.scale = (cfg.d_model // cfg.heads) ** -0.5
        self.cross = []
        for i in range(cfg.decoder_layers):
            lp = f"{self.p}layers.{i}.encoder_attn."
            k = _heads(_lin(enc_out, sd, lp + "k_proj", bias=False), cfg.heads)
            v = _heads(_lin(enc_out, sd, lp + "v_proj"), cfg.heads)
            self.cross.append((k, v))
        self.self_kv = [None] * cfg.decoder_layers
        self.pos = 0

    def reorder(self, idx):
        self.self_kv = [(k.index_select(0, idx), v.index_select(0, idx)) for (k, v) in self.self_kv]

    @torch.no_grad()
    def step(self, tokens):
        """tokens int64 [R, n] (n = prompt length on the first call, then 1) -> logits fp32 [R, V] of the last position
        (keep_dtype: in the dtype of the weights)."""
        sd, cfg, p = self.sd, self.cfg, self.p
        n = tokens.shape[1]
        x = sd[p + "embed_tokens.weight"][tokens] + sd[p + "embed_positions.weight"][self.pos:self.pos + n][None]
        mask = None
        if n > 1:
            mask = torch.full((n, self.pos + n), float("-inf"))
            mask = torch.triu(mask, diagonal=self.pos + 1)
        for i in range(cfg.decoder_layers):
            lp = f"{p}layers.{i}."
            r = x
            y = _ln(x, sd, lp + "self_attn_layer_norm")
            q = _heads(_lin(y, sd, lp + "self_attn.q_proj") * self.scale, cfg.heads)
            k = _heads(_lin(y, sd, lp + "self_attn.k_proj", bias=False), cfg.heads)
            v = _heads(_lin(y, sd, lp + "self_attn.v_proj"), cfg.heads)
            if self.self_kv[i] is not None:
                k = torch.cat([self.self_kv[i][0], k], dim=2)
                v = torch.cat([self.self_kv[i][1], v], dim=2)
            self.self_kv[i] = (k, v)
            x = r + _lin(_attn(q, k, v, mask), sd, lp + "self_attn.out_proj")
            r = x
            y = _ln(x, sd, lp + "encoder_attn_layer_norm")
            q = _heads(_lin(y, sd, lp + "encoder_attn.q_proj") * self.scale, cfg.heads)
            ck, cv = self.cross[i]
            x = r + _lin(_attn(q, ck, cv), sd, lp + "encoder_attn.out_proj")
            r = x
            y = _ln(x, sd, lp + "final_layer_norm")
            y = F.gelu(_lin(y, sd, lp + "fc1"))
            x = r + _lin(y, sd, lp + "fc2")
        self.pos += n
        x = _ln(x[:, -1], sd, p + "layer_norm")
        logits = F.linear(x, sd[p + "embed_tokens.weight"])
        return logits if self.keep_dtype else logits.float()


# ------------------------------------------------------------------------------------------------
# One decoding step, separated from the model: beam_step / greedy_step work on an explicit state and on logits of any origin;
# generate() is a loop over them.  The state has the fields of the device's decode state (include/wseg.h,
# wseg_debug_decode_step): S slots (windows being decoded), nb beams, R = S * nb rows (row = slot * nb + beam), L = max_length.
#
# Arithmetic: log-softmax in float64, rounded to float32; HF's masking and merging in float32, literally
# (generation/utils.py:3374-3452); the (cur_len + 1 - P) ** length_penalty denominators as Python floats.
# Selection: every choice is made with an explicit stable rule — on equal values the lower flat index wins (beam * V + token,
# then candidate rank, then "already finished before new") — never with torch.topk's order on ties.  Within one row the
# candidates are ranked by their processed logits (log-softmax and the row's running score are a shift of the whole row): where
# two distinct logits round to one float32 sum, HF's order is unspecified and the larger logit is taken.
_F32 = np.float32
_NEG = _F32(-1.0e9)
MAX_CAND = 16


class StepTrace:
    """What the reference decided in a step, for tests: `events` counts the paths taken, `decisions` lists every comparison
    between neighbours of a ranking that the result depends on, as (kind, gap, scale, denom, safe): gap = difference of the two
    float32 values (0: a tie, resolved by index), scale = the largest magnitude among the terms they were computed from (for a
    finished score c / denom: the terms of c, before the division), denom = the length-penalty denominator they were divided by
    (1 for the others), safe = both values are determined bit for bit
    whatever the summation order of the log-sum-exp (see _Val)."""

    def __init__(self):
        from collections import Counter
        self.events = Counter()
        self.decisions = []
        self.rows = []          # (row, token ids of its candidates best first + the next one, their processed logits)
        self.largest = {}       # ("cand", row, rank) / ("run_score", row) -> largest term; ("fin_score", row) -> (largest term of the
        #                         undivided score, denom, carried over unchanged)


class _Val:
    """A float32 score with what a margin check needs: `scale` (largest term), `denom`, and `src`: a key that is equal for two
    values computed by the same operations from bit-equal inputs (then any implementation gives them equal bits), or None;
    `exact`: the value does not depend on the rounding of the log-sum-exp at all."""
    __slots__ = ("v", "scale", "denom", "src", "exact")

    def __init__(self, v, scale, denom=1.0, src=None, exact=False):
        self.v, self.scale, self.denom, self.src, self.exact = _F32(v), float(scale), float(denom), src, bool(exact)


def _sticks_to_1e9(q):
    """-1e9 + q in float32 (spacing 64 there) is the same multiple of 64 for every q' within 1 of q."""
    d = (abs(float(q)) - 32.0) % 64.0
    return min(d, 64.0 - d) >= 1.0


def _rank(vals, k, trace, kind):
    """Indices of the k best of `vals` (_Val), value descending, on equal values the lower index first; records the decisions."""
    order = sorted(range(len(vals)), key=lambda i: (-float(vals[i].v), i))
    if trace is not None:
        for a, b in zip(order[:k], order[1:k + 1]):
            x, y = vals[a], vals[b]
            both_inf = np.isinf(x.v) and np.isinf(y.v)
            gap = 0.0 if both_inf else float(x.v) - float(y.v)
            safe = both_inf or (x.exact and y.exact) or (gap == 0.0 and x.src is not None and x.src == y.src)
            trace.decisions.append((kind, gap, max(x.scale, y.scale), min(x.denom, y.denom), safe))
            if gap == 0.0 and not both_inf:
                trace.events["tie_" + kind] += 1
    return order[:k]


@dataclass
class StepState:
    pos: np.ndarray
    done: np.ndarray
    win: np.ndarray
    wmax: np.ndarray
    unsat: np.ndarray
    tokens_in: np.ndarray
    run_score: np.ndarray
    fin_score: np.ndarray
    fin_flag: np.ndarray
    fin_len: np.ndarray
    run_seq: np.ndarray
    fin_seq: np.ndarray
    anc: np.ndarray
    cand_val: np.ndarray
    cand_tok: np.ndarray

    FIELDS = ("pos", "done", "win", "wmax", "unsat", "tokens_in", "run_score", "fin_score", "fin_flag", "fin_len", "run_seq",
              "fin_seq", "anc", "cand_val", "cand_tok")

    def copy(self):
        return StepState(**{f: getattr(self, f).copy() for f in self.FIELDS})


def new_state(n_slots, gp, wins=None, window_max_length=None, pos=None):
    """Freshly admitted slots: the prompt is in place and the slot stands at its last prompt position (`pos`: another one)."""
    S, nb, L, P = n_slots, gp.num_beams, gp.max_length, len(gp.prompt)
    R = S * nb
    seq = np.full((R, L), gp.pad_token_id, np.int32)
    seq[:, :P] = np.asarray(gp.prompt, np.int32)
    run_score = np.full((S, nb), _NEG, _F32)
    run_score[:, 0] = 0.0
    wins = np.arange(S, dtype=np.int32) if wins is None else np.asarray(wins, np.int32)
    wmax = np.full(S, L, np.int32)
    if window_max_length is not None:
        wmax = np.maximum(P + 1, np.minimum(L, np.asarray(window_max_length, np.int32)[wins])).astype(np.int32)
    p0 = P - 1 if pos is None else pos
    return StepState(pos=np.full(S, p0, np.int32), done=np.zeros(S, np.int32), win=wins, wmax=wmax, unsat=np.ones(S, np.int32),
                     tokens_in=np.full(R, gp.prompt[p0], np.int32), run_score=run_score.reshape(R),
                     fin_score=np.full(R, _NEG, _F32), fin_flag=np.zeros(R, np.int32), fin_len=np.zeros(R, np.int32),
                     run_seq=seq, fin_seq=seq.copy(), anc=np.tile(np.arange(nb, dtype=np.uint8).repeat(L), S).reshape(R, L),
                     cand_val=np.zeros((R, MAX_CAND), _F32), cand_tok=np.zeros((R, MAX_CAND), np.int32))


def _suppressed(V, cur_len, gp):
    m = np.zeros(V, bool)
    ids = list(gp.suppress_tokens) + (list(gp.begin_suppress_tokens) if cur_len == len(gp.prompt) else [])
    for t in ids:
        if 0 <= t < V:          # ids outside the vocabulary are ignored
            m[t] = True
    return m


def _row_candidates(x, sup, k):
    """Processed logits of one row (float32, suppressed -> -inf) and its k + 1 best ids, value descending, lower id first."""
    proc = np.where(sup, _F32(-np.inf), x.astype(_F32))
    n = min(k + 1, proc.shape[0])
    part = np.argpartition(-proc, n - 1)[:n] if n < proc.shape[0] else np.arange(proc.shape[0])
    kth = proc[part].min()
    pool = np.flatnonzero(proc >= kth)          # every id that ties with the (k + 1)-th value takes part: the lower id wins
    order = pool[np.lexsort((pool, -proc[pool].astype(np.float64)))][:n]
    return proc, order


def _log_softmax64(x):
    z = x.astype(np.float64)
    m = z.max()
    return (z - m) - math.log(np.exp(z - m).sum())


def _slots_of(state, slots):
    return range(state.pos.shape[0]) if slots is None else [int(w) for w in slots]


def beam_step(state, logits, gp, slots=None, trace=None, list_form=False):
    """One step of HF's _beam_search for every slot that is not done (`slots`: only those), in place.  logits [R, V]; with `slots`
    and list_form (the admission's form), [len(slots), V]: ONE row per listed slot, shared by its beams.
    Returns the flat source row of every row (which row's cache the new row continues; identity where nothing moved)."""
    nb, L, P, V = gp.num_beams, gp.max_length, len(gp.prompt), logits.shape[1]
    Kc = 2 * nb
    lp = float(gp.length_penalty)
    src_rows = np.arange(state.tokens_in.shape[0])
    for li, w in enumerate(_slots_of(state, slots)):
        if state.done[w]:
            continue
        pos = int(state.pos[w])
        cur_len = pos + 1
        rows = range(w * nb, (w + 1) * nb)
        if cur_len < P:                         # prompt phase: the next token is forced, nothing else changes
            state.tokens_in[w * nb:(w + 1) * nb] = gp.prompt[cur_len]
            state.pos[w] = pos + 1
            if trace is not None:
                trace.events["prompt_phase"] += 1
            continue
        sup = _suppressed(V, cur_len, gp)
        # a. / b. per row: log_softmax, suppress, + running score -> its Kc best
        cands = []                              # per beam: list of (_Val, token)
        for j, r in enumerate(rows):
            x = np.asarray(logits[li if list_form else r])
            proc, order = _row_candidates(x, sup, Kc)
            lsm = _log_softmax64(x)
            base = state.run_score[r]
            top2 = np.partition(x.astype(np.float64), -2)[-2:]
            dominated = bool(top2[1] - top2[0] >= 40.0)      # sum(exp(x - max)) rounds to 1.0f in any order: log-sum-exp == max exactly
            key = (x.tobytes(), float(base))
            row = []
            for t in order[:Kc]:
                l32 = _F32(lsm[t]) if not sup[t] else _F32(-np.inf)
                v = _F32(l32 + base)
                exact = (dominated and x[t] == top2[1]) or np.isinf(v) or (abs(float(base)) >= 1.0e8 and _sticks_to_1e9(l32))
                row.append((_Val(v, max(abs(float(l32)), abs(float(base)), abs(float(x[t]) - float(top2[1])), abs(float(v))), src=(key, float(x[t])), exact=exact), int(t)))
            cands.append(row)
            state.cand_val[r, :Kc] = [c[0].v for c in row]
            state.cand_tok[r, :Kc] = [c[1] for c in row]
            if trace is not None:
                trace.rows.append((r, [int(t) for t in order], proc[order].copy()))
                for rank, c in enumerate(row):
                    trace.largest[("cand", r, rank)] = c[0].scale
                if len(order) > Kc and sup[int(np.argmax(x))]:
                    trace.events["suppressed_row_max"] += 1
        # c. the Kc best continuations over the nb * V accumulated log-probs: flat index = beam * V + token
        flat = [(c[0], j, c[1]) for j, row in enumerate(cands) for c in row]      # already in flat-index order within equal values
        flat_vals = []
        for val, j, t in flat:
            fv = _Val(val.v, val.scale, src=None if val.src is None else (val.src[0], val.src[1]), exact=val.exact)
            flat_vals.append(fv)
        # two beams with bit-equal rows and scores give bit-equal candidates in any implementation: the tie is broken by the beam
        order = sorted(range(len(flat)), key=lambda i: (-float(flat[i][0].v), flat[i][1], i))
        if trace is not None:
            _rank([flat_vals[i] for i in order], Kc, trace, "beams")
        top = [flat[i] for i in order[:Kc]]
        c_val = [t[0] for t in top]
        c_beam = [t[1] for t in top]
        c_tok = [t[2] for t in top]
        if trace is not None:
            trace.events["tie_two_beams"] += any(c_val[k].v == c_val[k + 1].v and c_beam[k] != c_beam[k + 1] and not np.isinf(c_val[k].v)
                                                 for k in range(Kc - 1))
        # d. stopping criteria
        cap = cur_len + 1 >= int(state.wmax[w])
        c_hit = [(t == gp.eos_token_id) or cap for t in c_tok]
        # e. running beams for the next iteration
        run_val = []
        for k in range(Kc):
            if c_hit[k]:
                v = _F32(c_val[k].v + _F32(1.0) * _NEG)
                run_val.append(_Val(v, 1.0e9, exact=(abs(float(c_val[k].v)) < 1.0e6 and _sticks_to_1e9(c_val[k].v)) or c_val[k].exact or np.isinf(v)))
            else:
                run_val.append(_Val(c_val[k].v, c_val[k].scale, src=c_val[k].src, exact=c_val[k].exact))
        nxt = _rank(run_val, nb, trace, "running")
        # f. finished beams
        un = int(state.unsat[w])
        n_gen = cur_len + 1 - P
        denom = _F32(float(n_gen) ** lp)
        lp_exact = float(_F32(lp)) == lp
        merged = [_Val(state.fin_score[r], abs(float(state.fin_score[r])), exact=True) for r in rows]
        for k in range(Kc):
            did = c_hit[k] and k < nb
            v = _F32(c_val[k].v / denom)
            v = _F32(v + _F32(0.0) * _NEG)
            v = _F32(v + (_F32(0.0) if un else _F32(1.0)) * _NEG)
            v = _F32(v + (_F32(0.0) if did else _F32(1.0)) * _NEG)
            if un and did:
                merged.append(_Val(v, c_val[k].scale, denom=float(denom), exact=c_val[k].exact and lp_exact))      # scale: the terms of c, before the division
            else:
                merged.append(_Val(v, 1.0e9, exact=(abs(float(c_val[k].v) / float(denom)) < 1.0e6 and _sticks_to_1e9(float(c_val[k].v) / float(denom))) or np.isinf(v)))
        mi = _rank(merged, nb, trace, "finished")
        if trace is not None:
            trace.events["tie_finished_scores"] += any(un and c_hit[k] and k < nb and state.fin_flag[r] and merged[nb + k].v == state.fin_score[r]
                                                       for k in range(Kc) for r in rows)
        n_fin_score = [merged[m].v for m in mi]
        n_fin_flag = [int(state.fin_flag[w * nb + m]) if m < nb else int(c_hit[m - nb] and (m - nb) < nb) for m in mi]
        n_fin_len = [int(state.fin_len[w * nb + m]) if m < nb else n_gen for m in mi]
        # g. early-stop heuristic (early_stopping=False): can the best running beam still beat the worst finished one?
        best = run_val[nxt[0]]
        best_running = _F32(best.v / denom)
        mn = min(n_fin_score)
        improve = False
        wi = merged[mi[int(np.argmin(n_fin_score))]]
        for i in range(nb):
            worst = mn if n_fin_flag[i] else _NEG
            improve = improve or bool(best_running > worst)
            if trace is not None and un:
                safe = best.exact and lp_exact and (wi.exact or not n_fin_flag[i])
                trace.decisions.append(("early_stop", abs(float(best_running) - float(worst)),
                                        max(best.scale, wi.scale if n_fin_flag[i] else 0.0),
                                        min(float(denom), wi.denom if n_fin_flag[i] else 1.0e30), safe))
        un_new = int(bool(un) and improve)
        if trace is not None:
            ev = trace.events
            eos_ranks = [k for k in range(Kc) if c_tok[k] == gp.eos_token_id]
            ev["eos_rank_ge_nb_only"] += bool(eos_ranks) and min(eos_ranks) >= nb and not cap
            ev["eos_rank_0"] += bool(eos_ranks) and eos_ranks[0] == 0
            ev["eos_in_nb_rows"] += len([k for k in eos_ranks if k < nb]) >= nb
            ev["several_finish"] += sum(1 for k in range(nb) if c_hit[k]) >= 2 and bool(un)
            ev["cap_hit"] += cap
            ev["cap_at_first_step"] += cap and cur_len == P
            ev["unsat_already_0"] += not un
            ev["early_stop_improves"] += bool(un) and improve and any(n_fin_flag)
            ev["early_stop_stops"] += bool(un) and not improve and not cap
            ev["finished_new"] += any(m >= nb for m in mi)
            ev["begin_suppress_step"] += cur_len == P and bool(gp.begin_suppress_tokens)
        # write back
        old_run = state.run_seq[w * nb:(w + 1) * nb].copy()
        old_fin = state.fin_seq[w * nb:(w + 1) * nb].copy()
        old_anc = state.anc[w * nb:(w + 1) * nb].copy()
        state.unsat[w] = un_new
        if not un_new or cap:
            state.done[w] = 1
        else:
            state.pos[w] = pos + 1
        for i in range(nb):
            r = w * nb + i
            k = nxt[i]
            state.run_score[r] = run_val[k].v
            if trace is not None:
                trace.largest[("run_score", r)] = run_val[k].scale
                trace.largest[("fin_score", r)] = (merged[mi[i]].scale, merged[mi[i]].denom, mi[i] < nb)      # True: a stored score that was carried over
            state.fin_score[r] = n_fin_score[i]
            state.fin_flag[r] = n_fin_flag[i]
            state.fin_len[r] = n_fin_len[i]
            state.tokens_in[r] = c_tok[k]
            src_rows[r] = w * nb + c_beam[k]
            state.run_seq[r, :cur_len] = old_run[c_beam[k], :cur_len]
            state.run_seq[r, cur_len] = c_tok[k]
            state.run_seq[r, cur_len + 1:] = gp.pad_token_id
            state.anc[r, :cur_len] = old_anc[c_beam[k], :cur_len]
            state.anc[r, cur_len:] = i
            m = mi[i]
            if m < nb:
                state.fin_seq[r] = old_fin[m]
            else:
                state.fin_seq[r, :cur_len] = old_run[c_beam[m - nb], :cur_len]
                state.fin_seq[r, cur_len] = c_tok[m - nb]
                state.fin_seq[r, cur_len + 1:] = gp.pad_token_id
    return src_rows


def sampler_uniform24(seed, window, cur_len):
    """The counter-based generator of the sampler in Python integers: the top 24 bits of the splitmix64 finaliser of
    seed + 0x9E3779B97F4A7C15 * (window * 4096 + cur_len + 1)  (include/wseg.h, wseg_debug_decode_step)."""
    M = (1 << 64) - 1
    x = (seed + 0x9E3779B97F4A7C15 * (window * 4096 + cur_len + 1)) & M
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M
    x ^= x >> 31
    return x >> 40


def sample_candidate(vals, top_p, u24, info=None):
    """Index of the drawn candidate among `vals` (processed logits, best first, -inf = suppressed): HF's TopKLogitsWarper +
    TopPLogitsWarper + a draw with the uniform u24 / 2^24 scaled by the kept mass, in float32 as the product states it.
    info (dict): receives the distance of the uniform from the nearest cumulative boundary, relative to the kept mass."""
    with np.errstate(invalid="ignore"):
        pr = [_F32(np.exp(_F32(v - vals[0]))) if not np.isinf(v) else _F32(0.0) for v in vals]
    z = _F32(0.0)
    for q in pr:
        z = _F32(z + q)
    cut = 0.0 < top_p < 1.0
    kept = before = _F32(0.0)
    n_keep = 0
    for j, q in enumerate(pr):
        if j > 0 and (q <= 0.0 or (cut and before >= _F32(_F32(top_p) * z))):
            break
        kept = _F32(kept + q)
        before = _F32(before + q)
        n_keep += 1
    u = _F32(_F32(_F32(u24) * _F32(1.0 / 16777216.0)) * kept)
    acc = _F32(0.0)
    choice = n_keep - 1
    bounds = []
    for j in range(n_keep):
        acc = _F32(acc + pr[j])
        bounds.append(float(acc))
    for j in range(n_keep):
        if u < _F32(bounds[j]):
            choice = j
            break
    if info is not None:
        info["distance"] = min(abs(float(u) - b) for b in bounds) / float(kept)
        info["n_keep"] = n_keep
        info["cut_margin"] = min([abs(float(b) - float(_F32(_F32(top_p) * z))) / float(z) for b in bounds] or [1.0]) if cut else 1.0
    return choice


def greedy_step(state, logits, gp, slots=None, trace=None, list_form=False):
    """One greedy / sampling step (num_beams == 1) for every slot that is not done (`slots`: only those; list_form:
    logits [len(slots), V]), in place.  top_k <= 1: argmax of the processed logits, the lower id on equal values."""
    L, P, V = gp.max_length, len(gp.prompt), logits.shape[1]
    top_k = gp.top_k if gp.top_k > 1 else 1
    for li, w in enumerate(_slots_of(state, slots)):
        if state.done[w]:
            continue
        pos = int(state.pos[w])
        cur_len = pos + 1
        if cur_len < P:
            state.tokens_in[w] = gp.prompt[cur_len]
            state.pos[w] = pos + 1
            if trace is not None:
                trace.events["prompt_phase"] += 1
            continue
        x = np.asarray(logits[li if list_form else w])
        sup = _suppressed(V, cur_len, gp)
        proc, order = _row_candidates(x, sup, top_k)
        state.cand_val[w, :top_k] = proc[order[:top_k]]
        state.cand_tok[w, :top_k] = order[:top_k]
        if trace is not None:
            trace.rows.append((w, [int(t) for t in order], proc[order].copy()))
            if sup[int(np.argmax(x))]:
                trace.events["suppressed_row_max"] += 1
        tok = int(order[0])
        if top_k > 1:
            info = {} if trace is not None else None
            tok = int(order[sample_candidate(list(proc[order[:top_k]]), gp.top_p, sampler_uniform24(gp.seed, int(state.win[w]), cur_len), info)])
            if trace is not None:
                trace.decisions.append(("sample", min(info["distance"], info["cut_margin"]), 1.0, 1.0, False))
                trace.events["sample_cut"] += info["n_keep"] < top_k
        state.run_seq[w, cur_len] = tok
        state.anc[w, cur_len] = 0
        state.tokens_in[w] = tok
        cap = cur_len + 1 >= int(state.wmax[w])
        if tok == gp.eos_token_id or cap:
            state.unsat[w] = 0
            state.fin_len[w] = cur_len + 1 - P
            state.done[w] = 1
            if trace is not None:
                trace.events["cap_hit" if cap else "eos_rank_0"] += 1
        else:
            state.pos[w] = pos + 1
    return np.arange(state.tokens_in.shape[0])


def finalize(state, gp, slots=None):
    """Best sequence of each slot: (tokens [n, L] pad-filled, lengths [n]) — the product's retirement of a slot."""
    nb, L, P = gp.num_beams, gp.max_length, len(gp.prompt)
    ws = list(_slots_of(state, slots))
    toks = np.full((len(ws), L), gp.pad_token_id, np.int32)
    lens = np.zeros(len(ws), np.int32)
    for i, w in enumerate(ws):
        src = (state.run_seq if nb == 1 else state.fin_seq)[w * nb]
        lens[i] = P + int(state.fin_len[w * nb])
        toks[i, :lens[i]] = src[:lens[i]]
    return toks, lens


def run_loop(logits_fn, n_slots, gp, window_max_length=None, max_steps=None):
    """Steps freshly admitted slots until all are done.  logits_fn(state, src_rows) -> logits [R, V] for the rows' current
    tokens_in (src_rows: which row each row continues, None at the first call).  Returns (tokens, lengths, final state)."""
    state = new_state(n_slots, gp, window_max_length=window_max_length)
    step = greedy_step if gp.num_beams == 1 else beam_step
    src, n = None, 0
    while not state.done.all():
        src = step(state, logits_fn(state, src), gp)
        n += 1
        assert max_steps is None or n <= max_steps
    toks, lens = finalize(state, gp)
    return toks, lens, state


@torch.no_grad()
def generate(sd, cfg, feats, gp, return_first_logits=False):
    """feats [B,80,1000] -> int64 [B, L] token ids INCLUDING the prompt, padded with pad_token_id.

    Follows HF generate as the reference calls it (model.py:609-619): a loop of greedy_step / beam_step over the model's logits.
    A window that has finished is frozen while the others go on (HF stops stepping a batch once every item has finished).
    """
    B = feats.shape[0]
    nb = gp.num_beams
    enc = encoder_forward(sd, cfg, feats)
    dec = Decoder(sd, cfg, enc if nb == 1 else enc.repeat_interleave(nb, dim=0))
    P = len(gp.prompt)
    first = []

    def logits_fn(state, src):
        if src is None:
            inp = torch.from_numpy(state.run_seq[:, :P].astype(np.int64))
        else:
            dec.reorder(torch.from_numpy(src.astype(np.int64)))
            inp = torch.from_numpy(state.tokens_in.astype(np.int64))[:, None]
        logits = dec.step(inp)
        if not first:
            first.append(logits.clone())
        return logits.numpy()

    toks, lens, _ = run_loop(logits_fn, B, gp, window_max_length=gp.window_max_length)
    out = torch.from_numpy(toks[:, :int(lens.max())].astype(np.int64))
    return (out, first[0]) if return_first_logits else out


@torch.no_grad()
def score_sequence(sd, cfg, feats, gp, tokens):
    """HF's beam score of ONE given hypothesis for ONE window: sum of log_softmax(logits)[token] over the generated tokens
    (teacher-forced through the same decoder) / generated_length ** length_penalty — the quantity `_beam_search` ranks finished
    hypotheses by (HF generation/utils.py:3440-3452: topk_log_probs / (cur_len + 1 - prompt_len) ** length_penalty).
    feats [1,80,1000]; tokens: ids INCLUDING the prompt, up to and including EOS if there is one (pads stripped).
    Used by tests to show that a beam result that differs from the oracle's is an equally scored hypothesis (a near-tie
    resolved differently by another summation order), not an error."""
    P = len(gp.prompt)
    toks = [int(t) for t in tokens]
    assert toks[:P] == list(gp.prompt)
    gen = toks[P:]
    if gp.eos_token_id in gen:
        gen = gen[: gen.index(gp.eos_token_id) + 1]
    dec = Decoder(sd, cfg, encoder_forward(sd, cfg, feats))
    total = 0.0
    inp = torch.tensor([toks[:P]], dtype=torch.int64)
    for t in gen:
        lp = F.log_softmax(dec.step(inp), dim=-1)
        total += float(lp[0, t])
        inp = torch.tensor([[t]], dtype=torch.int64)
    return total / (len(gen) ** gp.length_penalty)


class TeacherForcer:
    """Encoder output and cross-attention K / V of ONE window in `dtype`, kept for any number of teacher_forced_logits-style passes."""

    @torch.no_grad()
    def __init__(self, sd, cfg, feats, dtype=torch.float64):
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.cfg = cfg
        self.enc = encoder_forward(self.sd, cfg, torch.as_tensor(feats).to(dtype).reshape(1, cfg.n_mels, -1))
        self.proto = Decoder(self.sd, cfg, self.enc, keep_dtype=True)

    @torch.no_grad()
    def logits(self, histories):
        hist = torch.as_tensor(histories, dtype=torch.int64)
        assert hist.dim() == 2 and 1 <= hist.shape[1] <= self.cfg.max_target_positions
        dec = Decoder.__new__(Decoder)      # a fresh self-attention cache on the shared cross K / V (they broadcast over the rows)
        dec.__dict__.update(self.proto.__dict__)
        dec.self_kv, dec.pos = [None] * self.cfg.decoder_layers, 0
        return dec.step(hist)


def teacher_forced_logits(sd, cfg, feats, histories, dtype=torch.float64):
    """Logits [rows, V] (in `dtype`, float64 by default) of the LAST position of given row histories of ONE window, teacher-forced
    through encoder + decoder as one causal pass in `dtype`: no decoding decisions, no cache bookkeeping, no beam reordering.
    feats [80, 1000] or [1, 80, 1000]; histories: token ids [rows, n], prompt included (the rows are independent).
    The float64 result is the reference for logits of late decode steps: the fp32 oracle is itself 2e-5 .. 4e-5 away from it on the
    fixture models, more than the split-precision modes are.  (TeacherForcer keeps the window's encoder output between calls.)"""
    return TeacherForcer(sd, cfg, feats, dtype).logits(histories)


def canonical(tokens, prompt_len, eos_token_id, prompt=None):
    """Generated ids up to and including the first EOS, prompt stripped (works for both HF
    conventions: 4.38.2 returns the prompt, 5.15 strips it)."""
    toks = [int(t) for t in tokens]
    if prompt is not None and toks[:len(prompt)] == list(prompt):
        toks = toks[len(prompt):]
    elif prompt is None:
        toks = toks[prompt_len:]
    out = []
    for t in toks:
        out.append(t)
        if t == eos_token_id:
            break
    return out


def random_state_dict(cfg, seed=0, std=0.02, dtype=torch.float32, fast=False):
    """Seeded random weights with HF parameter names (no checkpoints exist offline).

    fast=True tiles one 8M-sample normal pool instead of drawing every element (about 40x quicker for the
    1.5 B-parameter geometry); used only where the values do not matter (bench.py's cpu_baseline timing)."""
    g = torch.Generator().manual_seed(seed)
    d, f = cfg.d_model, cfg.ffn
    pool = torch.randn(1 << 23, generator=g) if fast else None
    pool2 = torch.cat([pool, pool]) if fast else None
    cursor = [0]

    def rn(*shape, s=std):
        if pool is None:
            return (torch.randn(*shape, generator=g) * s).to(dtype)
        n = 1
        for v in shape:
            n *= v
        reps = (n + pool.numel() - 1) // pool.numel() + 1
        start = cursor[0] % pool.numel()
        cursor[0] += 7919 + n
        flat = pool.repeat(reps)[start:start + n] if reps > 2 else pool2[start:start + n]
        return (flat.reshape(*shape) * s).to(dtype)

    sd = {}
    e = "model.encoder."
    sd[e + "conv1.weight"] = rn(d, cfg.n_mels, 3, s=0.05)
    sd[e + "conv1.bias"] = rn(d)
    sd[e + "conv2.weight"] = rn(d, d, 3)
    sd[e + "conv2.bias"] = rn(d)
    sd[e + "embed_positions.weight"] = rn(cfg.max_source_positions, d)

    def attn(prefix):
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[f"{prefix}{n}.weight"] = rn(d, d, s=d ** -0.5)
            if n != "k_proj":
                sd[f"{prefix}{n}.bias"] = rn(d)

    def ln(prefix):
        sd[prefix + ".weight"] = (1.0 + rn(d, s=0.1)).to(dtype)
        sd[prefix + ".bias"] = rn(d, s=0.1)

    def mlp(prefix):
        sd[prefix + "fc1.weight"] = rn(f, d, s=d ** -0.5)
        sd[prefix + "fc1.bias"] = rn(f)
        sd[prefix + "fc2.weight"] = rn(d, f, s=f ** -0.5)
        sd[prefix + "fc2.bias"] = rn(d)

    for i in range(cfg.encoder_layers):
        lp = f"{e}layers.{i}."
        attn(lp + "self_attn.")
        ln(lp + "self_attn_layer_norm")
        mlp(lp)
        ln(lp + "final_layer_norm")
    ln(e + "layer_norm")
    dd = "model.decoder."
    sd[dd + "embed_tokens.weight"] = rn(cfg.vocab_size, d, s=0.05)
    sd[dd + "embed_positions.weight"] = rn(cfg.max_target_positions, d, s=0.02)
    for i in range(cfg.decoder_layers):
        lp = f"{dd}layers.{i}."
        attn(lp + "self_attn.")
        ln(lp + "self_attn_layer_norm")
        attn(lp + "encoder_attn.")
        ln(lp + "encoder_attn_layer_norm")
        mlp(lp)
        ln(lp + "final_layer_norm")
    ln(dd + "layer_norm")
    return sd
