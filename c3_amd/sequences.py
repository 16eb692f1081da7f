"""Gate-sequence evaluation by index on the GPU: randomized benchmarking, ORBIT and the analytical error per Clifford.

The reference multiplies every sequence in a host loop (`evaluate_sequences`, c3/libraries/propagation.py:588-627) and
builds RB sequences gate name by gate name (`single_length_RB`, `inverseC`, c3/utils/qt_utils.py:448-491).  Here a
sequence list becomes ONE int32 index table into the table of gate propagators, and `c3p_seq_chain` evaluates all
P parameter samples x S sequences in one launch:

  {name: U [P,M,M]} + [[name, ...], ...]  --index table-->  c3p_seq_chain  -->  U_seq [P,S,M,M] | U_seq psi0 | population

RB and ORBIT only need |<0|U_seq|0>|^2, a chain of matrix-vector products (O(L M^2) per sequence, never O(L M^3)).

The single-qubit Clifford group is derived here, not tabulated: a breadth-first search over products of the ideal
rx90p, rx90m, ry90p, ry90m (c3/libraries/constants.py:52-56) modulo global phase gives each of the 24 Cliffords as a
shortest word; the identity is kept as rx90p rx90m, as the reference does, so no `Id` propagator is needed.  This table
is NOT the reference's `cliffords_decomp` (c3/utils/qt_utils.py:528-553): it is in another order, and two elements are
spelled with other words (the reference's C4 is ry90p rx90p rx90p, C16 ry90m rx90p rx90p).  With imperfect generators
the results depend on the words: a Clifford's actual propagator is the product of its word's actual gates, so
`epc_analytical` and `lindbladian_epc_analytical` from the generators change with the table, and RB / ORBIT sequences
from the same seed differ.  Every function that draws or spells Cliffords therefore takes `clifford_words` (24 lists of
generator names; `clifford_table`); a C3 binding passes c3.utils.qt_utils.cliffords_decomp for the reference's numbers,
and, with rng=None after the same np.random.seed, its exact RB sequences.  With `cliffords=True` (gates keyed C1..C24)
each supplied gate is paired with its ideal element by process fidelity (`match_cliffords`), so its numbering does not
matter.  `inverseC` takes and returns numbers into the table it is given.  DESIGN section 5.9 lists every difference from
the reference.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .fidelities import _super_overlap, fid_reg_deco, infid_sum
from .propagation import C3PropError, _Call, _is_torch, _ptr

MODES = {"product": 0, "state": 1, "population": 2}
GENERATORS = ("rx90p", "rx90m", "ry90p", "ry90m")


# ---------------------------------------------------------------------------------------------------------------------------
# the Clifford table
# ---------------------------------------------------------------------------------------------------------------------------
def _ideal_generators() -> Dict[str, np.ndarray]:
    """exp(-i pi/4 sigma) and its inverse for sigma = X, Y (the reference's GATES entries, constants.py:52-56)."""
    s = 1 / np.sqrt(2)
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
    I2 = np.eye(2, dtype=np.complex128)
    return {"rx90p": s * (I2 - 1j * X), "rx90m": s * (I2 + 1j * X), "ry90p": s * (I2 - 1j * Y), "ry90m": s * (I2 + 1j * Y)}


def _phase_key(U: np.ndarray) -> tuple:
    """U modulo global phase, as a hashable key: the phase of the largest entry (first one, row-major) set to 0."""
    flat = U.reshape(-1)
    k = int(np.argmax(np.abs(flat) > np.abs(flat).max() - 1e-9))
    V = flat * (abs(flat[k]) / flat[k])
    return tuple(np.round(np.concatenate([V.real, V.imag]), 8) + 0.0)


def word_matrix(word: Sequence[str], gates: Optional[Dict[str, np.ndarray]] = None) -> np.ndarray:
    """The matrix of a gate word, first gate applied first: G[w_{k-1}] ... G[w_0]."""
    gates = _ideal_generators() if gates is None else gates
    U = np.eye(2, dtype=np.complex128)
    for g in word:
        U = gates[g] @ U
    return U


def _derive_cliffords():
    gens = _ideal_generators()
    I2 = np.eye(2, dtype=np.complex128)
    words = {_phase_key(I2): ["rx90p", "rx90m"]}
    frontier = [([], I2)]
    while frontier:  # breadth-first: the first word that reaches an element is a shortest one
        nxt = []
        for word, U in frontier:
            for g in GENERATORS:
                V = gens[g] @ U
                k = _phase_key(V)
                if k not in words:
                    words[k] = word + [g]
                    nxt.append((word + [g], V))
        frontier = nxt
    table = list(words.values())
    if len(table) != 24:
        raise AssertionError(f"the Clifford search found {len(table)} elements, expected 24")
    return table, np.stack([word_matrix(w, gens) for w in table])


class CliffordTable:
    """The single-qubit Clifford group as 24 words over GENERATORS (first gate applied first), numbered in their order:
    `matrices` [24,2,2], `product[a, b]` = the index of C_b C_a (C_a applied first), `inverse[a]`, `identity`.
    Any decomposition of the group works; it is checked to give 24 distinct elements closed under products."""

    def __init__(self, words):
        gens = _ideal_generators()
        self.words = [list(w) for w in words]
        bad = [g for w in self.words for g in w if g not in GENERATORS]
        if len(self.words) != 24 or bad or not all(self.words):
            raise C3PropError(f"C3:Error: a Clifford table is 24 non-empty words over {GENERATORS}; got {len(self.words)} words"
                              + (f", unknown names {sorted(set(bad))}" if bad else ""))
        self.matrices = np.stack([word_matrix(w, gens) for w in self.words])
        self.index = {_phase_key(U): i for i, U in enumerate(self.matrices)}
        if len(self.index) != 24:
            raise C3PropError("C3:Error: the 24 Clifford words do not give 24 distinct elements")
        try:
            self.product = np.array([[self.index[_phase_key(self.matrices[b] @ self.matrices[a])] for b in range(24)] for a in range(24)], dtype=np.int64)
            self.identity = self.index[_phase_key(np.eye(2, dtype=np.complex128))]
        except KeyError:
            raise C3PropError("C3:Error: the 24 Clifford words are not closed under products (not the Clifford group)") from None
        self.inverse = np.array([int(np.argmax(self.product[a] == self.identity)) for a in range(24)], dtype=np.int64)


_TABLES = {}


def clifford_table(clifford_words=None) -> CliffordTable:
    """The table of `clifford_words` (24 lists of generator names, first applied first; None: this project's derived
    CLIFFORD_WORDS).  A C3 binding passes c3.utils.qt_utils.cliffords_decomp to number and spell the Cliffords as the
    reference does."""
    key = tuple(tuple(w) for w in (CLIFFORD_WORDS if clifford_words is None else clifford_words))
    if key not in _TABLES:
        _TABLES[key] = CliffordTable(key)
    return _TABLES[key]


CLIFFORD_WORDS, CLIFFORD_MATRICES = _derive_cliffords()
_DEFAULT = clifford_table()
_CLIFFORD_INDEX = _DEFAULT.index
_PRODUCT = _DEFAULT.product  # _PRODUCT[a, b] = index of C_b C_a (C_a applied first)
_INVERSE = _DEFAULT.inverse  # element 0 is the identity


def clifford_index(U: np.ndarray, clifford_words=None) -> int:
    """0-based index of an ideal 2x2 Clifford (any global phase) in the table of `clifford_words`."""
    return clifford_table(clifford_words).index[_phase_key(np.asarray(U, dtype=np.complex128))]


def inverseC(sequence, clifford_words=None) -> int:
    """qt_utils.py:480-491 on the table of `clifford_words` (default: this project's): the 1-based number of the
    Clifford that returns the product of `sequence` -- 1-based numbers into the same table, first applied first -- to
    the identity.  With the reference's words the numbers are its C1..C24."""
    tab = clifford_table(clifford_words)
    acc = tab.identity
    for c in sequence:
        acc = tab.product[acc, int(c) - 1]
    return int(tab.inverse[acc]) + 1


def _rng(rng):
    """None: numpy's global stream, as the reference; np.random itself, a Generator or a RandomState: used as given (so
    that a stream resolved once can be handed on); anything else: a seed."""
    if rng is None:
        return np.random
    if rng is np.random or isinstance(rng, (np.random.Generator, np.random.RandomState)):
        return rng
    return np.random.default_rng(rng)


def _rb_cliffords(RB_number: int, RB_length: int, rng, clifford_words=None) -> np.ndarray:
    """[RB_number, RB_length] 0-based Clifford indices: RB_length - 1 uniform draws and the recovery element.  One
    choice(24, size=(RB_number, RB_length - 1)) takes the same numbers from a stream as the reference's RB_number calls
    of size RB_length - 1 (qt_utils.py:470)."""
    tab = clifford_table(clifford_words)
    r = _rng(rng)
    body = r.choice(24, size=(RB_number, max(RB_length - 1, 0)))
    acc = np.full(RB_number, tab.identity, dtype=np.int64)
    for j in range(body.shape[1]):
        acc = tab.product[acc, body[:, j]]
    return np.concatenate([body, tab.inverse[acc][:, None]], axis=1)


def single_length_RB(RB_number: int, RB_length: int, target: int = 0, rng=None, clifford_words=None) -> List[List[str]]:
    """qt_utils.py:448-491: RB_number sequences of RB_length Cliffords (the last one the recovery), as gate keys
    "rx90p[target]" ...  `rng`: None (numpy's global generator, as the reference), a seed or a Generator.
    `clifford_words`: the decomposition the drawn numbers index (default: this project's table); with the reference's
    `cliffords_decomp` and rng=None the same np.random.seed gives the reference's sequences exactly."""
    words = clifford_table(clifford_words).words
    out = []
    for row in _rb_cliffords(RB_number, RB_length, rng, clifford_words):
        seq = []
        for c in row:
            seq.extend(f"{g}[{target}]" for g in words[c])
        out.append(seq)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the sequence chain
# ---------------------------------------------------------------------------------------------------------------------------
def index_table(sequences: Sequence[Sequence], gate_index: Dict[str, int]):
    """(seqs int32 [S, Lmax], lengths int32 [S]) for name sequences; unknown names raise."""
    S = len(sequences)
    lengths = np.fromiter((len(q) for q in sequences), dtype=np.int32, count=S)
    Lmax = int(lengths.max()) if S else 0
    seqs = np.zeros((S, Lmax), dtype=np.int32)
    for s, q in enumerate(sequences):
        try:
            seqs[s, : len(q)] = [gate_index[g] for g in q]
        except KeyError as e:
            raise C3PropError(f"C3:Error: sequence uses gate {e.args[0]!r} without a propagator") from None
    return seqs, lengths


def _psi0_arg(call, psi0, Pn: int, M: int):
    """(psi, per_sample): psi0 as [M] (any shape with M entries: one start vector for every sample) or [P,M] (one per sample)."""
    if psi0 is None:
        raise C3PropError("C3:Error: state mode needs psi0")
    psi = call.c128(psi0)
    n = 1
    for s in psi.shape:
        n *= int(s)
    if n == M:
        return psi.reshape(-1), False
    if psi.ndim == 2 and tuple(int(s) for s in psi.shape) == (Pn, M):
        return psi, True
    raise C3PropError(f"C3:Error: psi0 has shape {tuple(psi.shape)}; expected {M} entries or one start vector per sample [{Pn},{M}]")


def seq_chain(G, seqs, lengths, mode: str = "product", psi0=None, *, P: Optional[int] = None, superop: bool = False):
    """Direct binding of c3p_seq_chain.

    G [P, n_gates, M, M] (per-sample tables) or [n_gates, M, M] (one table for every sample; `P` then gives the number of
    samples, default 1); seqs int32 [S, Lmax]; lengths int32 [S].  numpy in -> numpy out (host pointers); CUDA tensors in
    -> CUDA tensors out, on the current stream.  Returns [P,S,M,M] (product), [P,S,M] (state) or [P,S] f64 (population).
    State mode: psi0 [M] starts every sample, psi0 [P,M] gives sample p its own start vector."""
    if mode not in MODES:
        raise C3PropError(f"C3:Error: unknown sequence mode {mode!r}; one of {sorted(MODES)}")
    call = _Call(G, psi0)
    Gt = call.c128(G)
    if Gt.ndim == 3:
        Pn, bstride = (1 if P is None else int(P)), 0
    elif Gt.ndim == 4:
        Pn = int(Gt.shape[0])
        if P is not None and int(P) != Pn:
            raise C3PropError(f"C3:Error: P={P} but the gate table has {Pn} samples")
        bstride = int(Gt.shape[1] * Gt.shape[2] * Gt.shape[3])
    else:
        raise C3PropError(f"C3:Error: gate table must be [n,M,M] or [P,n,M,M], got {tuple(Gt.shape)}")
    n, M = int(Gt.shape[-3]), int(Gt.shape[-1])
    if int(Gt.shape[-2]) != M:
        raise C3PropError(f"C3:Error: gates must be square, got {tuple(Gt.shape[-2:])}")
    if call.device:
        tt = call.torch
        sq = tt.as_tensor(seqs, device=call.dev).to(tt.int32).contiguous() if not _is_torch(seqs) else seqs.to(call.dev, tt.int32).contiguous()
        ln = tt.as_tensor(lengths, device=call.dev).to(tt.int32).contiguous() if not _is_torch(lengths) else lengths.to(call.dev, tt.int32).contiguous()
    else:
        sq = np.ascontiguousarray(seqs.cpu().numpy() if _is_torch(seqs) else seqs, dtype=np.int32)
        ln = np.ascontiguousarray(lengths.cpu().numpy() if _is_torch(lengths) else lengths, dtype=np.int32)
    if sq.ndim != 2 or ln.ndim != 1 or int(ln.shape[0]) != int(sq.shape[0]):
        raise C3PropError(f"C3:Error: seqs must be [S,Lmax] and lengths [S], got {tuple(sq.shape)} and {tuple(ln.shape)}")
    S, Lmax = int(sq.shape[0]), int(sq.shape[1])
    psi, psi_per_sample = None, False
    if mode == "state":
        psi, psi_per_sample = _psi0_arg(call, psi0, Pn, M)
    shape = {"product": (Pn, S, M, M), "state": (Pn, S, M), "population": (Pn, S)}[mode]
    if mode == "population":
        out = call.torch.empty(shape, dtype=call.torch.float64, device=call.dev) if call.device else np.empty(shape, dtype=np.float64)
    else:
        out = call.empty(shape)
    flags = call.flags | (_lib.SEQ_SUPEROP if superop else 0) | (_lib.SEQ_PSI0_PER_SAMPLE if psi_per_sample else 0)
    _lib.check(
        _lib.load().c3p_seq_chain(_ptr(Gt), bstride, n, M, Pn, _ptr(sq), S, Lmax, _ptr(ln), MODES[mode], _ptr(psi), flags, _ptr(out), call.stream)
    )
    return out


def seq_chain_vjp(G, seqs, lengths, mode: str, out_bar, psi0=None, *, P: Optional[int] = None, superop: bool = False, want_out: bool = False, want_psi0_bar: bool = False):
    """Direct binding of c3p_seq_chain_vjp: the cotangent of the gate table G from the cotangent `out_bar` of what
    `seq_chain(G, seqs, lengths, mode, psi0, P=P, superop=superop)` returns (d loss = Re sum conj(out_bar) d out).

    Returns G_bar with G's layout: [P, n_gates, M, M] for per-sample tables, [n_gates, M, M] (summed over the samples)
    for a shared one; with `want_out`, (G_bar, out) where out is the forward output of the same pass.  numpy in -> numpy
    out (host pointers); CUDA tensors in -> CUDA tensors out, on the current stream.

    State mode: psi0 is [M] or, one per sample, [P,M].  `want_psi0_bar` (state mode, c3p_seq_state_vjp) appends psi0_bar [P,M] to
    what is returned: the cotangent of the start vector per sample, also for a shared psi0 (sum over P then)."""
    if mode not in MODES:
        raise C3PropError(f"C3:Error: unknown sequence mode {mode!r}; one of {sorted(MODES)}")
    if want_psi0_bar and mode != "state":
        raise C3PropError("C3:Error: want_psi0_bar needs the state mode")
    call = _Call(G, psi0, out_bar)
    Gt = call.c128(G)
    if Gt.ndim == 3:
        Pn, bstride = (1 if P is None else int(P)), 0
    elif Gt.ndim == 4:
        Pn = int(Gt.shape[0])
        if P is not None and int(P) != Pn:
            raise C3PropError(f"C3:Error: P={P} but the gate table has {Pn} samples")
        bstride = int(Gt.shape[1] * Gt.shape[2] * Gt.shape[3])
    else:
        raise C3PropError(f"C3:Error: gate table must be [n,M,M] or [P,n,M,M], got {tuple(Gt.shape)}")
    n, M = int(Gt.shape[-3]), int(Gt.shape[-1])
    if int(Gt.shape[-2]) != M:
        raise C3PropError(f"C3:Error: gates must be square, got {tuple(Gt.shape[-2:])}")
    if call.device:
        tt = call.torch
        sq = tt.as_tensor(seqs, device=call.dev).to(tt.int32).contiguous() if not _is_torch(seqs) else seqs.to(call.dev, tt.int32).contiguous()
        ln = tt.as_tensor(lengths, device=call.dev).to(tt.int32).contiguous() if not _is_torch(lengths) else lengths.to(call.dev, tt.int32).contiguous()
    else:
        sq = np.ascontiguousarray(seqs.cpu().numpy() if _is_torch(seqs) else seqs, dtype=np.int32)
        ln = np.ascontiguousarray(lengths.cpu().numpy() if _is_torch(lengths) else lengths, dtype=np.int32)
    if sq.ndim != 2 or ln.ndim != 1 or int(ln.shape[0]) != int(sq.shape[0]):
        raise C3PropError(f"C3:Error: seqs must be [S,Lmax] and lengths [S], got {tuple(sq.shape)} and {tuple(ln.shape)}")
    S, Lmax = int(sq.shape[0]), int(sq.shape[1])
    psi, psi_per_sample = None, False
    if mode == "state":
        psi, psi_per_sample = _psi0_arg(call, psi0, Pn, M)
    shape = {"product": (Pn, S, M, M), "state": (Pn, S, M), "population": (Pn, S)}[mode]
    ob = call.f64(out_bar) if mode == "population" else call.c128(out_bar)
    if tuple(ob.shape) != shape:
        raise C3PropError(f"C3:Error: out_bar must be {list(shape)} for mode {mode!r}, got {list(ob.shape)}")
    out = None
    if want_out:
        if mode == "population":
            out = call.torch.empty(shape, dtype=call.torch.float64, device=call.dev) if call.device else np.empty(shape, dtype=np.float64)
        else:
            out = call.empty(shape)
    G_bar = call.empty((n, M, M) if bstride == 0 else (Pn, n, M, M))
    flags = call.flags | (_lib.SEQ_SUPEROP if superop else 0)
    if want_psi0_bar:
        psi_bar = call.empty((Pn, M))
        _lib.check(
            _lib.load().c3p_seq_state_vjp(
                _ptr(Gt), bstride, n, M, Pn, _ptr(sq), S, Lmax, _ptr(ln), _ptr(psi), M if psi_per_sample else 0, _ptr(ob), flags, _ptr(G_bar),
                _ptr(psi_bar), _ptr(out), call.stream
            )
        )
        return (G_bar, out, psi_bar) if want_out else (G_bar, psi_bar)
    flags |= _lib.SEQ_PSI0_PER_SAMPLE if psi_per_sample else 0
    _lib.check(
        _lib.load().c3p_seq_chain_vjp(
            _ptr(Gt), bstride, n, M, Pn, _ptr(sq), S, Lmax, _ptr(ln), MODES[mode], _ptr(psi), _ptr(ob), flags, _ptr(G_bar), _ptr(out), call.stream
        )
    )
    return (G_bar, out) if want_out else G_bar


def _gate_table(gate_Us: Dict):
    """names, G [P, n, M, M] (or [n, M, M] when every propagator is a single [M, M]) in the dict's order."""
    names = list(gate_Us.keys())
    vals = [gate_Us[k] for k in names]
    if any(_is_torch(v) for v in vals):
        import torch

        dev = next(v.device for v in vals if _is_torch(v))
        vals = [v.to(dev, torch.complex128) if _is_torch(v) else torch.as_tensor(np.asarray(v, dtype=np.complex128), device=dev) for v in vals]
        G = torch.stack(vals, dim=-3)
    else:
        G = np.stack([np.asarray(v, dtype=np.complex128) for v in vals], axis=-3)
    return names, G


def evaluate_sequences_indexed(gate_Us: Dict, sequences: Sequence[Sequence[str]], mode: str = "product", psi0=None, *, superop: bool = False):
    """`model_learning.evaluate_sequences_batch` by index: the same {name: U [P,M,M]} dict and name lists, one
    c3p_seq_chain launch.  Returns U_seq [P,S,M,M] (product), U_seq psi0 [P,S,M] (state) or the population of state 0
    [P,S] (|<0|U_seq|0>|^2; with `superop`, |(U_seq vec(|0><0|))[0]|).  Propagators given as [M,M] give P = 1.
    psi0 (state mode): [M], or [P,M] with one start vector per sample."""
    names, G = _gate_table(gate_Us)
    seqs, lengths = index_table(sequences, {k: i for i, k in enumerate(names)})
    return seq_chain(G, seqs, lengths, mode, psi0, superop=superop)


def evaluate_sequences_indexed_vjp(gate_Us: Dict, sequences: Sequence[Sequence[str]], mode: str, out_bar, psi0=None, *, superop: bool = False, want_out: bool = False, want_psi0_bar: bool = False):
    """Vector-Jacobian product of `evaluate_sequences_indexed` (same dict, name lists, mode and psi0): {name: U_bar}
    with each propagator's shape ([P,M,M], or [M,M] for unbatched input), from the cotangent `out_bar` of its output.
    One c3p_seq_chain_vjp launch.  With `want_out`: ({name: U_bar}, forward output).  psi0 (state mode) is [M] or [P,M];
    `want_psi0_bar` appends psi0_bar [P,M], the cotangent of the start vector per sample, to what is returned."""
    names, G = _gate_table(gate_Us)
    seqs, lengths = index_table(sequences, {k: i for i, k in enumerate(names)})
    unbatched = G.ndim == 3
    if unbatched:  # a [M,M] propagator per name is one sample (P = 1) with its own table: G_bar keeps its shape
        G = G[None]
    r = seq_chain_vjp(G, seqs, lengths, mode, out_bar, psi0, superop=superop, want_out=want_out, want_psi0_bar=want_psi0_bar)
    G_bar = r[0] if want_out or want_psi0_bar else r
    grads = {k: (G_bar[0, i] if unbatched else G_bar[:, i]) for i, k in enumerate(names)}
    if want_out or want_psi0_bar:
        return (grads,) + tuple(r[1:])
    return grads


# ---------------------------------------------------------------------------------------------------------------------------
# fidelities (c3/libraries/fidelities.py:437-591,754-791)
# ---------------------------------------------------------------------------------------------------------------------------
def _generator_keys(propagators: Dict, target=None) -> List[str]:
    """The propagator keys of rx90p, rx90m, ry90p, ry90m: "name[target]" (target found from the keys if None) or "name"."""
    keys = []
    for g in GENERATORS:
        if target is not None and f"{g}[{target}]" in propagators:
            keys.append(f"{g}[{target}]")
        elif g in propagators:
            keys.append(g)
        else:
            hits = [k for k in propagators if isinstance(k, str) and k.startswith(g + "[")] if target is None else []
            if len(hits) != 1:
                raise C3PropError(f"C3:Error: RB needs one propagator for {g} (target {target}); keys are {list(propagators)}")
            keys.append(hits[0])
    return keys


def _generator_table(propagators: Dict, target=None):
    """G [P, 4, M, M] (or [4, M, M]) of the four generators in GENERATORS order, and whether the input had no sample axis."""
    keys = _generator_keys(propagators, target)
    _, G = _gate_table({k: propagators[k] for k in keys})
    return G, G.ndim == 3


def _rb_index_table(cliffs: np.ndarray, clifford_words=None):
    """Clifford indices [S, n] (into the table of `clifford_words`) -> gate indices into GENERATORS order [S, Lmax] and
    lengths [S], fully vectorised."""
    word_idx = [np.array([GENERATORS.index(g) for g in w], dtype=np.int32) for w in clifford_table(clifford_words).words]
    wl = np.array([len(w) for w in word_idx], dtype=np.int32)
    pad = np.zeros((24, int(wl.max())), dtype=np.int32)
    for c, w in enumerate(word_idx):
        pad[c, : len(w)] = w
    lengths = wl[cliffs].sum(axis=1).astype(np.int32)
    S, Lmax = cliffs.shape[0], int(lengths.max()) if cliffs.size else 0
    seqs = np.zeros((S, Lmax), dtype=np.int32)
    take = np.arange(pad.shape[1])[None, None, :] < wl[cliffs][:, :, None]  # [S, n, wmax]
    gates = pad[cliffs]  # [S, n, wmax]
    for s in range(S):
        seqs[s, : lengths[s]] = gates[s][take[s]]
    return seqs, lengths


def _to_numpy(x):
    return x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)


def rb_survival(propagators: Dict, lengths: Sequence[int], num_seqs: int, *, lindbladian: bool = False, rng=None, target=None, clifford_words=None) -> np.ndarray:
    """Survival probabilities [P, n_lengths, num_seqs] of random Clifford sequences (RB_length Cliffords each, the last
    the recovery), every length and sequence in one population-mode call; the sequences are shared by the samples.
    The draws, length after length, are those of single_length_RB(num_seqs, L, rng=..., clifford_words=...)."""
    G, squeeze = _generator_table(propagators, target)
    r = _rng(rng)
    cl = [_rb_cliffords(num_seqs, int(L), r, clifford_words) for L in lengths]
    rows = []
    for c in cl:  # ragged Clifford counts -> per-sequence gate lists (padding is never read: lengths say how much is used)
        seqs, ln = _rb_index_table(c, clifford_words)
        rows.append((seqs, ln))
    Lmax = max(s.shape[1] for s, _ in rows)
    seqs = np.concatenate([np.pad(s, ((0, 0), (0, Lmax - s.shape[1]))) for s, _ in rows])
    ln = np.concatenate([l for _, l in rows])
    pop = _to_numpy(seq_chain(G, seqs, ln, "population", superop=lindbladian))
    return pop.reshape(pop.shape[0], len(lengths), num_seqs)


def _rb_lengths(min_length, max_length, num_lengths, logspace):
    if logspace:
        return np.rint(np.logspace(np.log10(min_length), np.log10(max_length), num=num_lengths)).astype(int)
    return np.rint(np.linspace(min_length, max_length, num=num_lengths)).astype(int)


def rb_fit(lengths, surv: np.ndarray):
    """The reference's fit (fidelities.py:548-560): A r^L + B to the mean survival per length, weighted by the standard
    error; bounds (0, 1), initial guess (0.9, 0.5, 0.5).  surv [n_lengths, num_seqs] -> (r, A, B); raises if it fails."""
    from scipy.optimize import curve_fit

    def RB_fit(L, r, A, B):
        return A * r**L + B

    means = np.mean(surv, axis=1)
    stds = np.std(surv, axis=1) / np.sqrt(surv.shape[1])
    solution, _ = curve_fit(RB_fit, np.asarray(lengths, dtype=np.float64), means, sigma=stds, bounds=(0, 1), p0=[0.9, 0.5, 0.5])
    return tuple(float(x) for x in solution)


@fid_reg_deco
def RB(propagators, min_length: int = 5, max_length: int = 500, num_lengths: int = 20, num_seqs: int = 30, logspace=False, lindbladian=False, padding="", *, rng=None, max_retries: int = 8, return_fit: bool = False, clifford_words=None):
    """fidelities.py:515-591 for every parameter sample: propagators {key: [P,M,M]} (or [M,M]) -> error per gate [P]
    (a float for unbatched input).  A sample whose fit fails is refitted, as in the reference, after adding num_lengths
    longer lengths (max_length + min_length .. 2 max_length, max_length doubling each time); after `max_retries` such
    rounds it raises instead of looping for ever.  `padding` is accepted for the signature and not used (single-qubit
    RB without idle padding).  `clifford_words`: the Clifford decomposition the sequences are drawn from (default: this
    project's table; the reference's `cliffords_decomp` with rng=None reproduces its draws).  With `return_fit`: (epg, r)
    arrays."""
    G, squeeze = _generator_table(propagators)
    r_ = _rng(rng)
    lengths = _rb_lengths(min_length, max_length, num_lengths, logspace)
    surv = rb_survival(propagators, lengths, num_seqs, lindbladian=lindbladian, rng=r_, clifford_words=clifford_words)
    P = surv.shape[0]
    rs = np.empty(P)
    for p in range(P):
        lens, sp, mx = lengths, surv[p], max_length
        for attempt in range(max_retries + 1):
            try:
                rs[p] = rb_fit(lens, sp)[0]
                break
            except Exception as message:  # noqa: BLE001 -- the reference retries on any failure of the fit
                if attempt == max_retries:
                    raise C3PropError(f"C3:Error: RB fit of sample {p} failed after {max_retries} extensions: {message}") from None
                new = _rb_lengths(mx + min_length, mx * 2, num_lengths, logspace)
                mx *= 2
                one = {k: (v[p] if not squeeze else v) for k, v in zip(GENERATORS, _unstack(G))}
                extra = rb_survival(one, new, num_seqs, lindbladian=lindbladian, rng=r_, clifford_words=clifford_words)[0]
                sp = np.concatenate([sp, extra])
                lens = np.append(lens, new)
    epc = 0.5 * (1 - rs)
    epg = 1 - ((1 - epc) ** (1 / 4))
    if squeeze:
        epg, rs = float(epg[0]), float(rs[0])
    return (epg, rs) if return_fit else epg


def _unstack(G):
    """G [P,4,M,M] or [4,M,M] -> the four generator blocks [P,M,M] / [M,M]."""
    return [G[..., i, :, :] for i in range(4)]


@fid_reg_deco
def lindbladian_RB_left(propagators: dict, gate: str = None, index=None, dims=None, proj: bool = False, clifford_words=None, **kw):
    """fidelities.py:594-603 on superoperators [P,D^2,D^2]: RB with the Lindblad population |(S vec(|0><0|))[0]|.  The
    reference calls RB without lindbladian=True, so it fits |(S vec(|0><0|))[0]|^2, and passes "left" as the target
    of single_length_RB; here the population is |.| and the target is found from the keys."""
    return RB(propagators, lindbladian=True, padding="left", clifford_words=clifford_words, **kw)


@fid_reg_deco
def lindbladian_RB_right(propagators: dict, gate: str = None, index=None, dims=None, proj: bool = False, clifford_words=None, **kw):
    """fidelities.py:606-608, as lindbladian_RB_left."""
    return RB(propagators, lindbladian=True, padding="right", clifford_words=clifford_words, **kw)


@fid_reg_deco
def orbit_infid(propagators, RB_number: int = 30, RB_length: int = 20, lindbladian=False, shots: int = None, seqs=None, noise=None, *, rng=None, clifford_words=None):
    """fidelities.py:754-791: mean over RB sequences of 1 - pop0, per parameter sample [P] (a float for unbatched input).
    The populations come from one population-mode call; with `shots`, each sequence's value is the mean of `shots`
    Bernoulli draws (one binomial draw on the host), and `noise` adds Gaussian noise per sequence, as the reference.
    `rng` (seed or Generator) makes both reproducible.  With `lindbladian` the propagators are superoperators and
    pop0 = |(S vec(|0><0|))[0]| (the reference computes |.|^2 of that entry whatever the flag).  Without `seqs` they
    are drawn by single_length_RB(RB_number, RB_length, rng=rng, clifford_words=clifford_words)."""
    r = _rng(rng)
    if not seqs:
        seqs = single_length_RB(RB_number=RB_number, RB_length=RB_length, rng=r, clifford_words=clifford_words)
    pop = _to_numpy(evaluate_sequences_indexed(propagators, seqs, "population", superop=bool(lindbladian)))
    p1 = np.clip(1.0 - pop, 0.0, 1.0) if shots else 1.0 - pop
    vals = r.binomial(int(shots), p1) / float(shots) if shots else p1
    if noise:
        vals = vals + r.standard_normal(vals.shape) * noise
    out = vals.mean(axis=-1)
    squeeze = all(np.ndim(v) == 2 for v in propagators.values())
    return float(out[0]) if squeeze else out


def orbit_infid_with_grad(propagators, RB_number: int = 30, RB_length: int = 20, lindbladian=False, seqs=None, *, rng=None, shots=None, noise=None, clifford_words=None):
    """`orbit_infid` and its gradient: (infid [P], {name: U_bar}) with d infid[p] = Re sum conj(U_bar[p]) dU[p] for every
    propagator (a float and [M,M] cotangents for unbatched input).  The value equals `orbit_infid` for the same `seqs`;
    both come from one population-mode c3p_seq_chain_vjp call.  `shots` and `noise` are random draws without a
    gradient and are refused."""
    if shots or noise:
        raise C3PropError("C3:Error: orbit_infid_with_grad has no gradient through `shots` / `noise` (random draws); "
                          "use orbit_infid for a sampled value")
    r = _rng(rng)
    if not seqs:
        seqs = single_length_RB(RB_number=RB_number, RB_length=RB_length, rng=r, clifford_words=clifford_words)
    squeeze = all(np.ndim(v) == 2 for v in propagators.values())
    P = 1 if squeeze else int(next(iter(propagators.values())).shape[0])
    S = len(seqs)
    # infid[p] = mean_s (1 - pop[p, s])  =>  pop_bar = -1 / S
    first = next(iter(propagators.values()))
    if _is_torch(first):
        import torch

        pop_bar = torch.full((P, S), -1.0 / S, dtype=torch.float64, device=first.device)
    else:
        pop_bar = np.full((P, S), -1.0 / S)
    grads, pop = evaluate_sequences_indexed_vjp(propagators, seqs, "population", pop_bar, superop=bool(lindbladian), want_out=True)
    out = (1.0 - _to_numpy(pop)).mean(axis=-1)
    return (float(out[0]) if squeeze else out), grads


def match_cliffords(U, rows, superop: bool = False, clifford_words=None) -> np.ndarray:
    """For 24 supplied Clifford propagators U [P,24,M,M] (numpy), the index into the table of `clifford_words` (default
    CLIFFORD_MATRICES) of the ideal element each
    one implements: the element of largest process fidelity on the computational block `rows` (2 row indices), averaged
    over the samples -- so a set keyed C1..C24 in ANY numbering (the reference's, this table's, a permutation) is paired
    with its own ideal gates.  For superoperators (`superop`) the block is the rows / columns i D + j of the computational
    pairs and the fidelity |tr(S super(C)^+)| / 4.  Distinct Cliffords have process fidelity <= 1/2 with each other, so the
    supplied gates must each be closer than that to exactly one ideal element, and all 24 elements must be met."""
    U = np.asarray(U)
    rows = np.asarray(rows, dtype=np.int64)
    CM = clifford_table(clifford_words).matrices
    if superop:
        D = int(round(np.sqrt(U.shape[-1])))
        idx = (rows[:, None] * D + rows[None, :]).reshape(-1)
        B = U[..., idx[:, None], idx[None, :]]  # [P,24,4,4]
        Cs = np.einsum("cij,ckl->cikjl", CM, CM.conj()).reshape(24, 4, 4)
        F = np.abs(np.einsum("pkij,cij->pkc", B, Cs.conj())) / 4
    else:
        B = U[..., rows[:, None], rows[None, :]]  # [P,24,2,2]
        F = np.abs(np.einsum("pkij,cij->pkc", B, CM.conj())) ** 2 / 4
    F = F.mean(axis=0)  # [24 supplied, 24 ideal]
    best = F.argmax(axis=1)
    if F.max(axis=1).min() <= 0.5 or len(set(best.tolist())) != 24:
        raise C3PropError("C3:Error: the propagators C1..C24 are not 24 distinct single-qubit Cliffords on the computational "
                          f"subspace (best process fidelities {np.round(F.max(axis=1), 3).tolist()})")
    return best


def clifford_products(propagators: Dict, cliffords: bool = False, target=None, *, rows=None, superop: bool = False, clifford_words=None):
    """(U [P,24,M,M], ideal [24]): the 24 Clifford propagators (product mode) and, for each, the index into the table of
    `clifford_words` (default CLIFFORD_MATRICES) of the ideal gate it stands for.  From the generators the products
    follow that table's words, so ideal[c] = c: the EPC averages over these products of the actual generators, and so
    depends on the words whenever the generators are not ideal.  With `cliffords` the propagators are keyed "C1".."C24"
    themselves; their numbering is not assumed to be the table's: each is paired with its ideal element by
    `match_cliffords` on the computational `rows`."""
    if cliffords:
        keys = [f"C{i}" for i in range(1, 25)]
        missing = [k for k in keys if k not in propagators]
        if missing:
            raise C3PropError(f"C3:Error: cliffords=True needs propagators keyed C1..C24; missing {missing}")
        U = evaluate_sequences_indexed({k: propagators[k] for k in keys}, [[k] for k in keys], "product")
        Un = _to_numpy(U)
        return U, match_cliffords(Un if Un.ndim == 4 else Un[None], rows, superop, clifford_words)
    keys = _generator_keys(propagators, target)
    name = dict(zip(GENERATORS, keys))
    words = clifford_table(clifford_words).words
    U = evaluate_sequences_indexed({k: propagators[k] for k in keys}, [[name[g] for g in w] for w in words], "product")
    return U, np.arange(24)


def _single_qubit_dims(index, dims):
    """The reference picks single- or two-qubit Cliffords from len(dims) (fidelities.py:440-446); only the single-qubit
    group is provided here, so more than one subsystem is refused rather than run on the wrong group."""
    dims = list(dims) if dims is not None else [2]
    index = list(index) if index is not None else [0]
    if len(dims) != 1 or len(index) != 1:
        raise C3PropError(f"C3:Error: analytical EPC is single-qubit here (dims {dims}, index {index}); the two-qubit "
                          "Clifford decomposition is not provided")
    return index, dims


def _per_clifford(U):
    """[P,24,M,M] -> 24 contiguous [P,M,M] blocks."""
    if _is_torch(U):
        Ut = U.transpose(0, 1).contiguous()
    else:
        Ut = np.ascontiguousarray(np.swapaxes(U, 0, 1))
    return [Ut[c] for c in range(24)]


@fid_reg_deco
def epc_analytical(propagators: dict, index, dims, proj: bool, cliffords=False, clifford_words=None):
    """fidelities.py:437-457 per parameter sample: 1 - mean over the 24 Cliffords of the average fidelity
    (c3p_gate_infid, kind = average, on the computational subspace of `index`).  [P] (a float for unbatched input).
    From the generators, the Cliffords are the products of the words of `clifford_words` (default: this project's table;
    the reference's `cliffords_decomp` gives its numbers); with imperfect generators the value depends on the words."""
    index, dims = _single_qubit_dims(index, dims)
    from .fidelities import computational_rows

    CM = clifford_table(clifford_words).matrices
    U, ideal = clifford_products(propagators, cliffords, rows=computational_rows(dims, index), clifford_words=clifford_words)
    infids = [_to_numpy(infid_sum(CM[ideal[c]], Uc, index, dims, kind="average", want_each=True)["each"]) for c, Uc in enumerate(_per_clifford(U))]
    out = np.mean(infids, axis=0)
    squeeze = all(np.ndim(v) == 2 for v in propagators.values())
    return float(out[0]) if squeeze else out


@fid_reg_deco
def lindbladian_epc_analytical(propagators: dict, index, dims, proj: bool, cliffords=False, clifford_words=None):
    """fidelities.py:460-480 per parameter sample, on superoperators [P,D^2,D^2]: the average fidelity of each Clifford
    from its process fidelity against tf_super(ideal), |(conj(t)/d + 1)/(d + 1)| with t = tr(S_c tf_super(C)^+) on
    the computational subspace (c3p_gate_overlap; d = 2).  `clifford_words` as in epc_analytical."""
    index, dims = _single_qubit_dims(index, dims)
    from .fidelities import computational_rows

    CM = clifford_table(clifford_words).matrices
    S, ideal = clifford_products(propagators, cliffords, rows=computational_rows(dims, index), superop=True, clifford_words=clifford_words)
    fids = []
    for c, Sc in enumerate(_per_clifford(S)):
        t, L = _super_overlap(CM[ideal[c]], Sc, index, dims)[:2]
        t = _to_numpy(t)
        fids.append(np.abs((np.conj(t) / L + 1) / (L + 1)))
    out = 1 - np.mean(fids, axis=0)
    squeeze = all(np.ndim(v) == 2 for v in propagators.values())
    return float(out[0]) if squeeze else out
