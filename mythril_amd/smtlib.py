"""SMT-LIB2 reader for Mythril's ``--solver-log`` dumps (``z3.Optimize.sexpr()``).

The reference writes one ``<hash>.smt2`` file per query (mythril/support/model.py:46-57):
``declare-fun`` lines, one ``assert`` per constraint, optional ``minimize``/``maximize``
directives and ``check-sat``.  This reader turns such a file into terms of
:mod:`mythril_amd.smt.terms`, which the engine lowers like any live query.  It understands
the z3 printer's forms: ``let`` bindings (``a!1`` …), ``(_ bvN w)`` / ``#x`` / ``#b``
literals, indexed operators (``(_ extract h l)``, ``(_ zero_extend n)``,
``(_ sign_extend n)``, ``(_ rotate_left n)``, ``(_ repeat n)``), ``(as const (Array …))``,
n-ary ``bvadd``/``bvmul``/``bvand``/``bvor``/``bvxor``/``concat``, z3's internal total
division names (``bvudiv_i`` …), ``bvumul_noovfl``, ``distinct``, ``=>``, and
``|quoted|`` symbols (``|keccak256_512-1|``).

Two things complete the path from a directory of dumps to the engine
(:mod:`mythril_amd.replay`): :func:`write_query`, a DAG printer in the same style (so this
project can write the files it reads), and :func:`recover_registry`, which rebuilds the
keccak part of a :class:`UFRegistry` from a query's own assertions — a file carries no
``KeccakFunctionManager``.
"""

from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

from .lower import LoweringError
from .smt import terms as T

_TOKEN = re.compile(r"\s*(?:(\()|(\))|(\|[^|]*\|)|(\"(?:[^\"]|\"\")*\")|([^\s()|\";]+)|(;[^\n]*))")


def tokenize(text: str):
    pos = 0
    n = len(text)
    while pos < n:
        m = _TOKEN.match(text, pos)
        if not m or m.end() == pos:
            if text[pos:].strip() == "":
                return
            raise ValueError(f"smtlib: cannot tokenize at {pos}: {text[pos:pos + 30]!r}")
        pos = m.end()
        if m.group(1):
            yield "("
        elif m.group(2):
            yield ")"
        elif m.group(3):
            yield m.group(3)
        elif m.group(4):
            yield m.group(4)
        elif m.group(5):
            yield m.group(5)


def parse_sexprs(text: str) -> list:
    stack: list = [[]]
    for tok in tokenize(text):
        if tok == "(":
            stack.append([])
        elif tok == ")":
            top = stack.pop()
            stack[-1].append(top)
        else:
            stack[-1].append(tok)
    if len(stack) != 1:
        raise ValueError("smtlib: unbalanced parentheses")
    return stack[0]


def _sym(tok: str) -> str:
    return tok[1:-1] if tok.startswith("|") and tok.endswith("|") else tok


@dataclass
class Query:
    assertions: List[T.Term] = field(default_factory=list)
    minimize: List[T.Term] = field(default_factory=list)
    maximize: List[T.Term] = field(default_factory=list)
    decls: Dict[str, tuple] = field(default_factory=dict)

    @property
    def objective_free(self) -> bool:
        return not self.minimize and not self.maximize


def _sort(s) -> tuple:
    if s == "Bool":
        return T.BOOL
    if isinstance(s, list) and s[:2] == ["_", "BitVec"]:
        return T.bv_sort(int(s[2]))
    if isinstance(s, list) and s and s[0] == "Array":
        d, r = _sort(s[1]), _sort(s[2])
        return T.array_sort(d[1], r[1])
    raise LoweringError(f"smtlib: unsupported sort {s}")


_NARY = {"bvadd": "bvadd", "bvmul": "bvmul", "bvand": "bvand", "bvor": "bvor", "bvxor": "bvxor"}
_BIN = {
    "bvsub": "bvsub", "bvudiv": "bvudiv", "bvurem": "bvurem", "bvsdiv": "bvsdiv",
    "bvsrem": "bvsrem", "bvsmod": "bvsmod", "bvudiv_i": "bvudiv", "bvurem_i": "bvurem",
    "bvsdiv_i": "bvsdiv", "bvsrem_i": "bvsrem", "bvsmod_i": "bvsmod", "bvshl": "bvshl",
    "bvlshr": "bvlshr", "bvashr": "bvashr",
    "bvexp": "bvexp",   # the facade's own exponentiation term (write_query prints it by this name)
}
_CMPS = {
    "bvult": ("bvult", False), "bvule": ("bvule", False), "bvslt": ("bvslt", False),
    "bvsle": ("bvsle", False), "bvugt": ("bvult", True), "bvuge": ("bvule", True),
    "bvsgt": ("bvslt", True), "bvsge": ("bvsle", True), "bvumul_noovfl": ("bvumul_noovfl", False),
}
# overflow predicates of SMT-LIB 2.7 (newer z3 prints them): name -> (no-overflow form, negate)
_OVFL = {
    "bvuaddo": ("bvuadd_noovfl", True), "bvumulo": ("bvumul_noovfl", True),
    "bvusubo": ("bvult", False),
}


_EVAL, _LET, _RESTORE, _APPLY = range(4)
_UNBOUND = object()


class Reader:
    def __init__(self):
        self.q = Query()
        self.funs: Dict[str, Tuple[List[tuple], tuple]] = {}

    def read(self, text: str) -> Query:
        for cmd in parse_sexprs(text):
            if not isinstance(cmd, list) or not cmd:
                continue
            head = cmd[0]
            if head == "declare-fun":
                name = _sym(cmd[1])
                doms = [_sort(s) for s in cmd[2]]
                rng = _sort(cmd[3])
                self.funs[name] = (doms, rng)
                self.q.decls[name] = (tuple(doms), rng)
            elif head == "declare-const":
                name = _sym(cmd[1])
                self.funs[name] = ([], _sort(cmd[2]))
                self.q.decls[name] = ((), _sort(cmd[2]))
            elif head == "define-fun" and not cmd[2]:
                name = _sym(cmd[1])
                self.funs[name] = ([], _sort(cmd[3]))
                self._defs = getattr(self, "_defs", {})
                self._defs[name] = self.term(cmd[4], {})
            elif head == "assert":
                self.q.assertions.append(self.term(cmd[1], {}))
            elif head == "minimize":
                self.q.minimize.append(self.term(cmd[1], {}))
            elif head == "maximize":
                self.q.maximize.append(self.term(cmd[1], {}))
            # set-info / set-option / check-sat / get-model / exit: ignored
        return self.q

    # ---- terms ---------------------------------------------------------------------------
    def term(self, e, env: Dict[str, T.Term]) -> T.Term:
        """One s-expression as a term, without recursion: z3 prints every shared subterm as a
        nested ``let`` (``a!1`` …), so a large dump nests thousands deep.  An explicit work
        stack evaluates it on the caller's thread at any depth (the recursive
        reader had to re-run on a big-stack thread under a raised process-wide recursion
        limit, which made deep recursion on other threads segfault meanwhile).

        ``let`` is parallel (the bindings see the outer scope) and scoped: the bound names
        are set in one mutable environment for the body and restored after it."""
        env = dict(env)
        vals: List[T.Term] = []
        work: list = [(_EVAL, e)]
        while work:
            kind, x = work.pop()
            if kind == _EVAL:
                if isinstance(x, str):
                    vals.append(self._atom(x, env))
                    continue
                head = x[0]
                if head == "_" and len(x) == 3 and x[1].startswith("bv") and x[1][2:].isdigit():
                    vals.append(T.const(int(x[1][2:]), int(x[2])))  # (_ bvN w) literal
                    continue
                if head == "let":
                    work.append((_LET, x))
                    for binding in reversed(x[1]):
                        work.append((_EVAL, binding[1]))
                    continue
                work.append((_APPLY, x))
                for a in reversed(x[1:]):
                    work.append((_EVAL, a))
            elif kind == _LET:          # the bindings' values are on the stack: the body
                names = [_sym(b[0]) for b in x[1]]
                bound = vals[len(vals) - len(names):]
                del vals[len(vals) - len(names):]
                undo = [(nm, env.get(nm, _UNBOUND)) for nm in names]
                for nm, v in zip(names, bound):
                    env[nm] = v
                work.append((_RESTORE, undo))
                work.append((_EVAL, x[2]))
            elif kind == _RESTORE:      # leave the let's scope
                for nm, old in reversed(x):
                    if old is _UNBOUND:
                        env.pop(nm, None)
                    else:
                        env[nm] = old
            else:                       # _APPLY: the arguments are on the stack
                n = len(x) - 1
                args = vals[len(vals) - n:] if n else []
                del vals[len(vals) - n:]
                head = x[0]
                if isinstance(head, list):
                    vals.append(self._indexed(head, args))
                    continue
                h = _sym(head)
                if h in self.funs:
                    doms, rng = self.funs[h]
                    if rng[0] != "bv":
                        raise LoweringError(f"smtlib: UF {h} with range {rng}")
                    vals.append(T.apply(h, rng[1], *args))
                else:
                    vals.append(apply_named(h, args))
        return vals[0]

    def _atom(self, tok: str, env) -> T.Term:
        s = _sym(tok)
        if s in env:
            return env[s]
        if tok == "true":
            return T.TRUE
        if tok == "false":
            return T.FALSE
        if tok.startswith("#x"):
            return T.const(int(tok[2:], 16), 4 * (len(tok) - 2))
        if tok.startswith("#b"):
            return T.const(int(tok[2:], 2), len(tok) - 2)
        defs = getattr(self, "_defs", {})
        if s in defs:
            return defs[s]
        if s in self.funs:
            doms, rng = self.funs[s]
            if doms:
                raise LoweringError(f"smtlib: {s} used without arguments")
            if rng == T.BOOL:
                return T.boolvar(s)
            if rng[0] == "bv":
                return T.var(s, rng[1])
            return T.array(s, rng[1], rng[2])
        raise LoweringError(f"smtlib: unknown symbol {s}")

    def _indexed(self, head: list, args: List[T.Term]) -> T.Term:
        if head[0] == "_":
            return apply_indexed(head[1], [int(p) for p in head[2:]], args)
        if head[0] == "as" and head[1] == "const":
            srt = _sort(head[2])
            return T.const_array(srt[1], args[0])
        raise LoweringError(f"smtlib: unsupported indexed operator {head}")


def apply_named(h: str, args: List[T.Term]) -> T.Term:
    """An interpreted SMT-LIB2 / z3 operator applied to terms (shared by the text reader and
    the z3-AST walker, mythril_amd/z3_terms.py)."""
    if h in _NARY:
        acc = args[0]
        for a in args[1:]:
            acc = T.binop(_NARY[h], acc, a)
        return acc
    if h in _BIN:
        return T.binop(_BIN[h], args[0], args[1])
    if h == "bvneg":
        return T.bvneg(args[0])
    if h == "bvnot":
        return T.bvnot(args[0])
    if h in _CMPS:
        op, swap = _CMPS[h]
        a, b = (args[1], args[0]) if swap else (args[0], args[1])
        return T.cmp(op, a, b)
    if h in _OVFL:
        # SMT-LIB 2.7 overflow predicates (true iff the operation overflows)
        op, neg = _OVFL[h]
        r = T.cmp(op, args[0], args[1])
        return T.not_(r) if neg else r
    if h == "bvnand":
        return T.bvnot(T.binop("bvand", args[0], args[1]))
    if h == "bvnor":
        return T.bvnot(T.binop("bvor", args[0], args[1]))
    if h == "bvxnor":
        return T.bvnot(T.binop("bvxor", args[0], args[1]))
    if h == "bvcomp":
        return T.ite(T.eq(args[0], args[1]), T.const(1, 1), T.const(0, 1))
    if h == "concat":
        return T.concat(*args)
    if h == "=":
        if len(args) == 2:
            return T.eq(args[0], args[1])
        return T.and_(*[T.eq(args[i], args[i + 1]) for i in range(len(args) - 1)])
    if h == "distinct":
        return T.and_(*[T.not_(T.eq(args[i], args[j]))
                        for i in range(len(args)) for j in range(i + 1, len(args))])
    if h in ("ite", "if"):
        return T.ite(args[0], args[1], args[2])
    if h == "and":
        return T.and_(*args)
    if h == "or":
        return T.or_(*args)
    if h == "not":
        return T.not_(args[0])
    if h == "xor":
        acc = args[0]
        for a in args[1:]:
            acc = T.xor(acc, a)
        return acc
    if h == "=>":
        return T.or_(T.not_(args[0]), args[1])
    if h == "select":
        return T.select(args[0], args[1])
    if h == "store":
        return T.store(args[0], args[1], args[2])
    raise LoweringError(f"smtlib: unsupported operator {h}")


def apply_indexed(op: str, params: List[int], args: List[T.Term]) -> T.Term:
    """``((_ op p...) args)`` — extract / zero_extend / sign_extend / repeat / rotations."""
    if op == "extract":
        return T.extract(params[0], params[1], args[0])
    if op == "zero_extend":
        return T.zero_extend(params[0], args[0])
    if op == "sign_extend":
        n = params[0]
        a = args[0]
        if n == 0:
            return a
        msb = T.extract(a.width - 1, a.width - 1, a)
        fill = T.ite(T.eq(msb, T.const(1, 1)), T.const(-1, n), T.const(0, n))
        return T.concat(fill, a)
    if op == "repeat":
        return T.concat(*([args[0]] * params[0]))
    if op in ("rotate_left", "rotate_right"):
        a, k = args[0], params[0] % args[0].width
        if k == 0:
            return a
        w = a.width
        if op == "rotate_right":
            k = w - k
        return T.concat(T.extract(w - 1 - k, 0, a), T.extract(w - 1, w - k, a))
    raise LoweringError(f"smtlib: unsupported indexed operator {op}")


def read_query(text: str) -> Query:
    """One --solver-log query.  z3 prints shared subterms as nested ``let`` bindings, so a
    large dump nests thousands deep: the reader's term walk is iterative (Reader.term)."""
    return Reader().read(text)


def read_file(path: str) -> Query:
    with open(path) as f:
        return read_query(f.read())


# ---- writer: the z3 printer's style, shared subterms as let bindings ----------------------
# written bare; anything else is quoted, which is always valid (|keccak256_512-1|, |1_calldata|)
_SIMPLE_SYMBOL = re.compile(r"^[A-Za-z_][0-9A-Za-z_.]*$")
_RESERVED = frozenset(
    ["let", "as", "_", "par", "forall", "exists", "match", "true", "false", "not", "and", "or",
     "xor", "ite", "if", "=", "=>", "distinct", "select", "store", "concat", "bvneg", "bvnot",
     "bvnand", "bvnor", "bvxnor", "bvcomp"]
    + list(_NARY) + list(_BIN) + list(_CMPS) + list(_OVFL))
_LEAF_OPS = ("bv", "true", "false", "var", "bvar", "array")


def quote_symbol(name: str) -> str:
    """``name`` as an SMT-LIB2 symbol: as is when it is a simple symbol that no operator or
    reserved word claims, ``|quoted|`` otherwise (``1_calldatasize``, ``keccak256_512-1``)."""
    name = str(name)
    if _SIMPLE_SYMBOL.match(name) and name not in _RESERVED:
        return name
    if "|" in name or "\\" in name:
        raise ValueError(f"smtlib: {name!r} cannot be written as a symbol")
    return f"|{name}|"


def literal(value: int, w: int) -> str:
    """A bit-vector literal as z3 prints it: ``#x…`` for widths divisible by 4, else
    ``(_ bvN w)``."""
    value &= T.M(w)
    return f"#x{value:0{w // 4}x}" if w % 4 == 0 else f"(_ bv{value} {w})"


def _sort_str(sort: tuple) -> str:
    if sort == T.BOOL:
        return "Bool"
    if sort[0] == "bv":
        return f"(_ BitVec {sort[1]})"
    return f"(Array (_ BitVec {sort[1]}) (_ BitVec {sort[2]}))"


def declaration_lines(roots) -> List[str]:
    """``declare-fun`` lines of every free symbol and UF under ``roots``, in first-occurrence
    order (the z3 printer's)."""
    out, seen, done = [], set(), set()
    stack = list(reversed(list(roots)))
    while stack:
        t = stack.pop()
        if t in done:
            continue
        done.add(t)
        if t.op in ("var", "bvar", "array"):
            if t.val not in seen:
                seen.add(t.val)
                out.append(f"(declare-fun {quote_symbol(t.val)} () {_sort_str(t.sort)})")
        elif t.op == "apply":
            name, doms = t.val
            if not doms:
                raise ValueError(f"smtlib: application of {name} without arguments")
            if name not in seen:
                seen.add(name)
                d = " ".join(f"(_ BitVec {w})" for w in doms)
                out.append(f"(declare-fun {quote_symbol(name)} ({d}) (_ BitVec {t.width}))")
        stack.extend(reversed(t.args))
    return out


def _open(t: T.Term) -> Tuple[str, str]:
    """(text before the operands, text after them) of a non-leaf term.  Every form reads
    back, through :func:`apply_named` / :func:`apply_indexed`, as the same constructor call on
    the same operands — hence as the identical hash-consed term."""
    op = t.op
    if op == "extract":
        return f"((_ extract {t.val[0]} {t.val[1]})", ")"
    if op == "zero_extend":
        return f"((_ zero_extend {t.val})", ")"
    if op == "K":
        return f"((as const (Array (_ BitVec {t.sort[1]}) (_ BitVec {t.sort[2]})))", ")"
    if op == "apply":
        return f"({quote_symbol(t.val[0])}", ")"
    if op == "iff":
        return "(=", ")"
    if op == "bvuadd_noovfl":
        # z3 has no name for it; SMT-LIB 2.7's overflow predicate, negated, is the same term
        return "(not (bvuaddo", "))"
    return f"({op}", ")"


def _leaf(t: T.Term) -> str:
    if t.op == "bv":
        return literal(t.val, t.width)
    if t.op in ("true", "false"):
        return t.op
    return quote_symbol(t.val)


def _expr_text(root: T.Term, prefix: str) -> str:
    """One term, subterms used more than once bound by nested ``let``s as ``<prefix>N``."""
    if root.op in _LEAF_OPS:
        return _leaf(root)
    # post-order over the DAG; uses counts operand slots, so a term used twice by one parent
    # is shared too
    uses: Dict[T.Term, int] = {}
    order: List[T.Term] = []
    stack = [(root, False)]
    while stack:
        t, done = stack.pop()
        if done:
            order.append(t)
            continue
        if t in uses:
            uses[t] += 1
            continue
        uses[t] = 1
        if t.op in _LEAF_OPS:
            continue
        stack.append((t, True))
        for a in reversed(t.args):
            stack.append((a, False))
    shared = {t for t in order if uses[t] > 1 and t is not root}
    # let level of a term: the longest chain of shared subterms below it; a binding of level
    # k only names bindings of lower levels, so one parallel let per level is well scoped
    level: Dict[T.Term, int] = {}
    for t in order:
        lv = 0
        for a in t.args:
            if a.op not in _LEAF_OPS:
                lv = max(lv, level[a] + (1 if a in shared else 0))
        level[t] = lv
    names: Dict[T.Term, str] = {}
    by_level: Dict[int, List[T.Term]] = {}
    for t in sorted((t for t in order if t in shared), key=lambda t: level[t]):   # stable
        names[t] = f"{prefix}{len(names) + 1}"
        by_level.setdefault(level[t], []).append(t)

    def body(t: T.Term, out: List[str]) -> None:
        """``t`` written out, shared subterms by name (iterative: store chains run deep)."""
        work: list = [t]
        first = True
        while work:
            x = work.pop()
            if isinstance(x, str):
                out.append(x)
                continue
            if x.op in _LEAF_OPS:
                out.append(_leaf(x))
                continue
            if x in names and not first:
                out.append(names[x])
                continue
            first = False
            head, tail = _open(x)
            out.append(head)
            work.append(tail)
            for a in reversed(x.args):
                work.append(a)
                work.append(" ")

    out: List[str] = []
    depth = 0
    for lv in sorted(by_level):
        pad = "  " * depth
        out.append(f"{pad}(let (")
        for i, t in enumerate(by_level[lv]):
            out.append(("" if i == 0 else f"\n{pad}      ") + f"({names[t]} ")
            body(t, out)
            out.append(")")
        out.append(")\n")
        depth += 1
    out.append("  " * depth)
    body(root, out)
    out.append(")" * depth)
    return "".join(out)


def write_query(constraints, minimize=(), maximize=(), style: str = "z3") -> str:
    """The query as SMT-LIB2 text in the z3 printer's style: ``declare-fun`` lines in
    first-occurrence order, one ``assert`` per constraint with per-assert
    ``(let ((a!1 …)) …)`` bindings for the subterms used more than once (a DAG, where
    ``Optimize.sexpr()`` prints the tree), ``#x…`` literals for widths divisible by 4 and
    ``(_ bvN w)`` otherwise, ``|quoted|`` names where needed, the ``minimize`` /
    ``maximize`` lines and ``(check-sat)``.

    ``read_query(write_query(cs)).assertions[i] is cs[i]``: every form is the reader's own
    spelling of the constructor that made the term."""
    if style != "z3":
        raise ValueError(f"smtlib: unknown style {style!r}")
    cs = [c.raw if hasattr(c, "raw") else c for c in constraints]
    mins = [c.raw if hasattr(c, "raw") else c for c in minimize]
    maxs = [c.raw if hasattr(c, "raw") else c for c in maximize]
    lines = declaration_lines(cs + mins + maxs)
    # let names must not shadow a declared symbol: z3's a!N, with more '!' while one does
    prefix = "a!"
    declared = [ln.split(" ", 2)[1].strip("|") for ln in lines]
    while any(n.startswith(prefix) for n in declared):
        prefix += "!"
    for head, terms in (("assert", cs), ("minimize", mins), ("maximize", maxs)):
        for c in terms:
            text = _expr_text(c, prefix)
            lines.append(f"({head} {text})" if "\n" not in text else f"({head}\n{text})")
    return "\n".join(lines) + "\n(check-sat)\n"


# ---- the keccak registry of a dump, from its own assertions -------------------------------
_KECCAK_FN = re.compile(r"^keccak256_(\d+)$")


@dataclass
class Recovery:
    """What :func:`recover_registry` saw besides the registry it returns."""

    symbolic: Dict[int, int] = field(default_factory=dict)       # width -> symbolic inputs
    ambiguous: Dict[int, List[int]] = field(default_factory=dict)  # width -> the lo values met
    dropped: List[Tuple[int, int, int]] = field(default_factory=list)  # (width, k, h): not keccak

    def problems(self, registry) -> List[str]:
        """Why a query with this recovery cannot be searched: a width with symbolic inputs
        whose interval is ambiguous or missing."""
        out = [f"keccak256_{n}: ambiguous interval ({len(los)} different lower bounds)"
               for n, los in sorted(self.ambiguous.items())]
        for n in sorted(self.symbolic):
            spec = registry.keccak.get(n)
            if n not in self.ambiguous and (spec is None or spec.lo is None):
                out.append(f"keccak256_{n}: no interval recovered for its symbolic inputs")
        return out


def _keccak_app(t: T.Term):
    """The width n when ``t`` is an application ``keccak256_<n>(x)``, else None."""
    if t.op == "apply" and len(t.args) == 1:
        m = _KECCAK_FN.match(t.val[0])
        if m and t.args[0].width == int(m.group(1)):
            return int(m.group(1))
    return None


def _eq_app_const(t: T.Term):
    """(application, constant) of ``f(x) == const`` written either way round, else None."""
    if t.op == "=":
        a, b = t.args
        if b.op == "bv" and _keccak_app(a) is not None:
            return a, b
        if a.op == "bv" and _keccak_app(b) is not None:
            return b, a
    return None


def _ule_spelled_out(t: T.Term):
    """(lo, application) of ``or(bvult(const lo, f(x)), const lo == f(x))`` — the facade's
    ``ULE`` (``Or(ULT, ==)``, as the reference's bitvec_helper spells it) — with the
    disjuncts and the sides of ``=`` in either order; else None."""
    if t.op != "or" or len(t.args) != 2:
        return None
    for lt, eq in (t.args, t.args[::-1]):
        if lt.op == "bvult" and lt.args[0].op == "bv" and _keccak_app(lt.args[1]) is not None:
            hit = _eq_app_const(eq)
            if hit is not None and hit[0] is lt.args[1] and hit[1] is lt.args[0]:
                return lt.args[0].val, lt.args[1]
    return None


def keccak_message(k: int, n: int) -> bytes:
    """The bytes the analysis hashes for input value ``k`` of width ``n``
    (``KeccakFunctionManager.find_concrete_keccak``)."""
    return k.to_bytes(n // 8, "big")


def verify_pairs(pairs, engine=None) -> List[bool]:
    """Whether each ``(n, k, h)`` is a real hash, ``h == Keccak-256(k as n/8 bytes)``, by ONE
    batched ``engine.keccak256`` call."""
    pairs = list(pairs)
    ok = [n % 8 == 0 and n > 0 for n, _, _ in pairs]
    idx = [i for i, good in enumerate(ok) if good]
    if idx:
        if engine is None:
            from . import engine as E

            engine = E.get_engine()
        digests = engine.keccak256([keccak_message(pairs[i][1], pairs[i][0]) for i in idx])
        for i, d in zip(idx, digests):
            ok[i] = int.from_bytes(bytes(d), "big") == pairs[i][2]
    return ok


def drop_unverified(registry, ok_of) -> None:
    """Remove the concrete pairs that ``ok_of(n, k, h)`` rejects (a width left with neither
    an interval nor a pair loses its entry); they are listed in ``registry.recovery.dropped``."""
    for n in list(registry.keccak):
        spec = registry.keccak[n]
        for k in [k for k, h in spec.concrete.items() if not ok_of(n, k, h)]:
            registry.recovery.dropped.append((n, k, spec.concrete.pop(k)))
        if spec.lo is None and not spec.concrete:
            del registry.keccak[n]


def recover_registry(assertions, verify: bool = True, engine=None):
    """The keccak part of a :class:`UFRegistry`, rebuilt from a query's own assertions: the
    shapes ``KeccakFunctionManager._create_condition`` / ``create_conditions`` emit
    (mythril_amd/keccak_manager.py), met anywhere under nested ``and`` / ``or``.

    * Interval: ``bvule(const lo, f(x))`` — or the same spelled out, as the facade's ``ULE``
      does, ``or(bvult(lo, f(x)), lo == f(x))`` — and ``bvult(f(x), const hi)`` on the same
      application ``f = keccak256_<n>(x)`` with ``hi - lo == PART`` set ``keccak[n].lo``.  All
      symbolic inputs of a width share one interval: two different ``lo`` leave the width
      without an entry, listed in ``.recovery.ambiguous``.
    * Concrete hashes: ``and(f(x) == const h, const k == x)`` and ``f(const k) == const h``
      (either side order of ``=``) give ``concrete[k] = h``.  With ``verify`` every pair is
      checked by one batched ``engine.keccak256`` call and a pair that is not the real
      Keccak-256 of ``k`` at width ``n`` is dropped (``.recovery.dropped``); a caller with
      many queries passes ``verify=False`` and checks them all at once
      (:func:`verify_pairs`, :func:`drop_unverified`).
    * Widths whose functions appear only as ``keccak256_<n>-1``, or not at all, get no
      entry; ``actors`` stay the default.

    The returned registry carries a :class:`Recovery` as ``.recovery``.

    Recovery decides only what the search can find: it fixes the interpretation of
    ``keccak256_<n>`` the candidates are built under.  It is not a soundness gate — every
    witness is still re-checked on the host against the file's own assertions, interval
    conditions included, as for any query."""
    from .keccak_manager import PART
    from .smt.to_dag import KeccakSpec, UFRegistry

    rec = Recovery()
    lows: Dict[T.Term, set] = {}     # application -> lower bounds met
    highs: Dict[T.Term, set] = {}    # application -> upper bounds met
    concrete: Dict[int, Dict[int, int]] = {}
    seen = set()
    junctions = []                   # the and / or skeleton of the assertions
    stack = list(assertions)
    while stack:                     # one walk of the DAG: symbolic inputs, and the skeleton
        t = stack.pop()
        if t in seen:
            continue
        seen.add(t)
        n = _keccak_app(t)
        if n is not None and t.args[0].op != "bv":
            rec.symbolic[n] = rec.symbolic.get(n, 0) + 1
        stack.extend(t.args)
    seen = set()
    stack = list(assertions)
    while stack:
        t = stack.pop()
        if t in seen:
            continue
        seen.add(t)
        if t.op in ("and", "or"):
            lo_app = _ule_spelled_out(t)
            if lo_app is not None:
                lows.setdefault(lo_app[1], set()).add(lo_app[0])
                continue
            junctions.append(t)
            stack.extend(t.args)
            continue
        if t.op == "bvule" and t.args[0].op == "bv" and _keccak_app(t.args[1]) is not None:
            lows.setdefault(t.args[1], set()).add(t.args[0].val)
        elif t.op == "bvult" and t.args[1].op == "bv" and _keccak_app(t.args[0]) is not None:
            highs.setdefault(t.args[0], set()).add(t.args[1].val)
        else:
            hit = _eq_app_const(t)
            if hit is not None and hit[0].args[0].op == "bv":     # f(const k) == const h
                app, h = hit
                concrete.setdefault(_keccak_app(app), {})[app.args[0].val] = h.val
    for j in junctions:
        if j.op != "and":
            continue
        for c in j.args:             # and(f(x) == const h, const k == x)
            hit = _eq_app_const(c)
            if hit is None:
                continue
            app, h = hit
            x = app.args[0]
            for d in j.args:
                if d.op == "=" and d is not c:
                    a, b = d.args
                    k = a if (b is x and a.op == "bv") else b if (a is x and b.op == "bv") else None
                    if k is not None:
                        concrete.setdefault(_keccak_app(app), {})[k.val] = h.val
    los: Dict[int, set] = {}
    for app, ls in lows.items():
        for lo in ls:
            if (lo + PART) in highs.get(app, ()):
                los.setdefault(_keccak_app(app), set()).add(lo)
    reg = UFRegistry()
    reg.recovery = rec
    for n in sorted(set(los) | set(concrete)):
        if len(los.get(n, ())) > 1:
            rec.ambiguous[n] = sorted(los[n])
            continue
        lo = next(iter(los[n])) if n in los else None
        reg.keccak[n] = KeccakSpec(lo=lo, concrete=dict(sorted(concrete.get(n, {}).items())))
    if verify:
        triples = [(n, k, h) for n, s in reg.keccak.items() for k, h in s.concrete.items()]
        good = dict(zip(triples, verify_pairs(triples, engine)))
        drop_unverified(reg, lambda n, k, h: good[(n, k, h)])
    return reg


def registry_signature(registry) -> tuple:
    """What distinguishes two recovered registries: ``lo`` per width plus the concrete
    pairs."""
    return tuple((n, s.lo, tuple(sorted(s.concrete.items()))) for n, s in sorted(registry.keccak.items()))
