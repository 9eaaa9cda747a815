"""Column expressions: `df.x`, `df["x"]`, `col("x")`, arithmetic, comparisons,
`&` / `|` / `~`, `.alias()`, `.cast()`, `.asc()` / `.desc()`.

A `Column` is a small expression tree over the columns of a frame. It holds
no data; `DataFrame.select` / `withColumn` / `filter` compile it, through the
graph builder (graph/dsl.py), into ONE GraphDef with one placeholder per
referenced column (built like `core.block`, so analyzed shape metadata is
honoured) and run it with the engine: a chain of comparisons and arithmetic
becomes one fused elementwise kernel.

Dtype rules (no silent promotion, as everywhere in the engine): a Python
scalar takes the dtype of the column it meets; a float scalar against an
integer column, or two columns of different dtypes, raise
`InvalidTypeException` (the user writes `.cast(...)`). Cells may be scalars or
fixed-shape arrays; a column of lower cell rank broadcasts over the cells of
the other (a scalar column against a vector column compares row by row), and
`.sum()` / `.min()` / `.max()` / `.mean()` / `.all()` / `.any()` reduce over
the cell, which is how a predicate over a vector column yields one value per
row.

`.asc()` / `.desc()` mark a Column as a sort order for `DataFrame.orderBy` /
`sort` / `sortWithinPartitions`; such a Column is no value: `select`,
`withColumn`, `filter` and every operator refuse it (`InvalidTypeException`).
"""
from __future__ import annotations

import numbers
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..utils import dtypes as D
from .column_info import ColumnInformation
from .types import DataType, NumericType, StructField, StructType, sql_type_from_string

_ARITH = {"add": "+", "sub": "-", "mul": "*", "div": "/"}
_COMPARE = {"eq": "=", "ne": "!=", "lt": "<", "le": "<=", "gt": ">", "ge": ">="}
_LOGICAL = {"and": "AND", "or": "OR"}
_REDUCE = ("sum", "min", "max", "mean", "all", "any")


def _errors():
    from .. import core
    return core


def _type_name(dt: Optional[int]) -> str:
    return "?" if dt is None else D.dtype_name(dt)


def _is_literal(v) -> bool:
    return isinstance(v, (numbers.Number, np.generic, np.ndarray)) and not isinstance(v, Column)


class Column:
    """An expression over the columns of a DataFrame (see the module docstring)."""

    __slots__ = ("_expr", "_alias", "_order")
    __hash__ = None  # `==` builds an expression: columns are not hashable

    def __init__(self, expr: tuple, alias: Optional[str] = None, order: Optional[str] = None):
        self._expr = expr
        self._alias = alias
        self._order = order  # "asc" / "desc": a sort order (orderBy / sort / sortWithinPartitions only)

    # -- construction
    @staticmethod
    def _ref(name: str, field: Optional[StructField] = None) -> "Column":
        dt = rank = None
        if field is not None:
            stf = ColumnInformation(field).stf
            if stf is not None:
                dt, rank = stf.tf_dtype, max(stf.shape.num_dims - 1, 0)
        return Column(("ref", name, dt, rank))

    def alias(self, name: str) -> "Column":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return Column(self._expr, name, self._order)

    name = alias

    def cast(self, to) -> "Column":
        """`to`: a numeric SQL type or "double" | "float" | "int" | "bigint"."""
        self._no_sort_order("cast")
        t = sql_type_from_string(to) if isinstance(to, str) else to
        if isinstance(t, type) and issubclass(t, DataType):
            t = t()
        if not isinstance(t, NumericType):
            raise _errors().InvalidTypeException(
                f"cast: unsupported type {to!r}; use a numeric SQL type or one of double, float, int, bigint")
        return Column(("cast", self._expr, t.tf_dtype), self._alias)

    astype = cast

    # -- sort orders
    def asc(self) -> "Column":
        """This expression as an ascending sort key (NaN after +inf, -0.0 == 0.0)."""
        return Column(self._expr, self._alias, "asc")

    def desc(self) -> "Column":
        """This expression as a descending sort key."""
        return Column(self._expr, self._alias, "desc")

    @property
    def sort_order(self) -> Optional[str]:
        """"asc" / "desc" for a Column made by .asc() / .desc(), else None."""
        return self._order

    def _no_sort_order(self, where: str) -> None:
        if self._order is not None:
            raise _errors().InvalidTypeException(
                f"{where}: '{self.output_name}.{self._order}()' is a sort order, not a value; it is accepted only "
                f"by orderBy / sort / sortWithinPartitions")

    # -- naming
    @property
    def is_reference(self) -> bool:
        """A plain column reference (aliased or not): selected without a copy."""
        return self._expr[0] == "ref"

    @property
    def output_name(self) -> str:
        return self._alias if self._alias is not None else _describe(self._expr)

    def __repr__(self):
        return f"Column<{self.output_name}>"

    # -- operators
    def _binary(self, op: str, other, reflected: bool = False) -> "Column":
        self._no_sort_order(f"operator '{_ARITH.get(op) or _COMPARE.get(op) or _LOGICAL[op]}'")
        if isinstance(other, Column):
            other._no_sort_order(f"operator '{_ARITH.get(op) or _COMPARE.get(op) or _LOGICAL[op]}'")
            o = other._expr
        elif _is_literal(other):
            o = ("lit", other)
        else:
            return NotImplemented
        expr = ("bin", op, o, self._expr) if reflected else ("bin", op, self._expr, o)
        _typeof(expr, None)  # what is already known is checked now
        return Column(expr)

    def __add__(self, o):
        return self._binary("add", o)

    def __radd__(self, o):
        return self._binary("add", o, True)

    def __sub__(self, o):
        return self._binary("sub", o)

    def __rsub__(self, o):
        return self._binary("sub", o, True)

    def __mul__(self, o):
        return self._binary("mul", o)

    def __rmul__(self, o):
        return self._binary("mul", o, True)

    def __truediv__(self, o):
        return self._binary("div", o)

    def __rtruediv__(self, o):
        return self._binary("div", o, True)

    def __neg__(self):
        self._no_sort_order("unary '-'")
        expr = ("un", "neg", self._expr)
        _typeof(expr, None)
        return Column(expr)

    def __eq__(self, o):  # noqa: D105
        return self._binary("eq", o)

    def __ne__(self, o):
        return self._binary("ne", o)

    def __lt__(self, o):
        return self._binary("lt", o)

    def __le__(self, o):
        return self._binary("le", o)

    def __gt__(self, o):
        return self._binary("gt", o)

    def __ge__(self, o):
        return self._binary("ge", o)

    def __and__(self, o):
        return self._binary("and", o)

    def __rand__(self, o):
        return self._binary("and", o, True)

    def __or__(self, o):
        return self._binary("or", o)

    def __ror__(self, o):
        return self._binary("or", o, True)

    def __invert__(self):
        self._no_sort_order("operator '~'")
        expr = ("un", "not", self._expr)
        _typeof(expr, None)
        return Column(expr)

    def __bool__(self):
        raise ValueError("Cannot convert column into bool: please use '&' for 'and', '|' for 'or', "
                         "'~' for 'not' when building DataFrame boolean expressions.")

    def _reduce(self, op: str) -> "Column":
        self._no_sort_order(f"{op}()")
        expr = ("red", op, self._expr)
        _typeof(expr, None)
        return Column(expr)

    def sum(self) -> "Column":  # noqa: A003
        """Sum over each cell (one value per row)."""
        return self._reduce("sum")

    def min(self) -> "Column":  # noqa: A003
        return self._reduce("min")

    def max(self) -> "Column":  # noqa: A003
        return self._reduce("max")

    def mean(self) -> "Column":
        return self._reduce("mean")

    def all(self) -> "Column":  # noqa: A003
        """True where every element of a boolean cell is true."""
        return self._reduce("all")

    def any(self) -> "Column":  # noqa: A003
        return self._reduce("any")


def col(name: str) -> Column:
    """An unbound column reference, resolved against the frame it is used on."""
    if not isinstance(name, str):
        raise TypeError(f"col: a column name is expected, got {name!r}")
    return Column._ref(name)


column = col


def asc(name: str) -> Column:
    """`col(name).asc()`: an ascending sort key for orderBy / sort / sortWithinPartitions."""
    return col(name).asc()


def desc(name: str) -> Column:
    """`col(name).desc()`: a descending sort key."""
    return col(name).desc()


# ------------------------------------------------------------------ analysis
def _describe(e: tuple) -> str:
    k = e[0]
    if k == "ref":
        return e[1]
    if k == "lit":
        v = e[1]
        return repr(v.tolist()) if isinstance(v, (np.ndarray, np.generic)) else repr(v)
    if k == "un":
        return ("(- " if e[1] == "neg" else "(NOT ") + _describe(e[2]) + ")"
    if k == "cast":
        return f"CAST({_describe(e[1])} AS {D.dtype_name(e[2])})"
    if k == "red":
        return f"{e[1]}({_describe(e[2])})"
    sym = _ARITH.get(e[1]) or _COMPARE.get(e[1]) or _LOGICAL[e[1]]
    return f"({_describe(e[2])} {sym} {_describe(e[3])})"


def references(e: tuple, out: Optional[List[str]] = None) -> List[str]:
    """Names of the columns an expression reads, in first-use order."""
    out = [] if out is None else out
    if e[0] == "ref":
        if e[1] not in out:
            out.append(e[1])
    else:
        for a in e[1:]:
            if isinstance(a, tuple):
                references(a, out)
    return out


def _field_info(schema: StructType, name: str) -> Tuple[int, int]:
    core = _errors()
    if name not in schema:
        raise core.TensorFramesError(f"Could not find column with name {name}; available columns: "
                                     f"{', '.join(schema.names)}")
    f = schema[name]
    stf = ColumnInformation(f).stf
    if stf is None:
        raise core.TensorFramesError(f"The datatype of column '{name}' could not be understood by "
                                     f"tensorframes: {f.dataType}")
    return stf.tf_dtype, max(stf.shape.num_dims - 1, 0)


def _check_literal(v, dt: Optional[int], what: str) -> None:
    if dt is None:
        return
    core = _errors()
    kind = np.asarray(v).dtype.kind
    if dt == D.DT_BOOL:
        if kind != "b":
            raise core.InvalidTypeException(f"{what}: a boolean expression meets the non-boolean value {v!r}")
        return
    if kind == "b":
        raise core.InvalidTypeException(f"{what}: the boolean value {v!r} meets a column of type {_type_name(dt)}")
    if kind == "c" or (kind == "f" and not D.as_dtype(dt).is_floating):
        raise core.InvalidTypeException(
            f"{what}: the value {v!r} is not of the column's type {_type_name(dt)} (a scalar takes the dtype of "
            f"the column it meets); use .cast(\"double\") on the column")


def _typeof(e: tuple, schema: Optional[StructType]) -> Tuple[Optional[int], Optional[int]]:
    """(tf dtype, cell rank) of an expression; None where not known yet (an
    unbound `col()` before it meets its frame: schema is None). Raises
    InvalidTypeException for what is known to be wrong."""
    core = _errors()
    k = e[0]
    if k == "ref":
        if schema is not None:
            return _field_info(schema, e[1])
        return e[2], e[3]
    if k == "lit":
        return None, np.asarray(e[1]).ndim
    if k == "cast":
        _, r = _typeof(e[1], schema)
        return e[2], r
    if k == "un":
        dt, r = _typeof(e[2], schema)
        if dt is not None and e[1] == "not" and dt != D.DT_BOOL:
            raise core.InvalidTypeException(f"{_describe(e)}: '~' needs a boolean expression, got {_type_name(dt)}")
        if dt is not None and e[1] == "neg" and dt == D.DT_BOOL:
            raise core.InvalidTypeException(f"{_describe(e)}: unary '-' on a boolean expression; use '~'")
        return dt, r
    if k == "red":
        dt, _ = _typeof(e[2], schema)
        if dt is not None and (e[1] in ("all", "any")) != (dt == D.DT_BOOL):
            raise core.InvalidTypeException(
                f"{_describe(e)}: {e[1]}() over a {_type_name(dt)} expression; all()/any() reduce boolean cells, "
                f"sum()/min()/max()/mean() numeric ones")
        return dt, 0
    op, a, b = e[1], e[2], e[3]
    what = _describe(e)
    (da, ra), (db, rb) = _typeof(a, schema), _typeof(b, schema)
    if a[0] == "lit":
        _check_literal(a[1], db, what)
        da = db
    elif b[0] == "lit":
        _check_literal(b[1], da, what)
        db = da
    elif da is not None and db is not None and da != db:
        raise core.InvalidTypeException(
            f"{what}: '{_describe(a)}' is {_type_name(da)} but '{_describe(b)}' is {_type_name(db)}; "
            f"no implicit conversion, use .cast(...) on one of them")
    dt = da if da is not None else db
    rank = None if ra is None or rb is None else max(ra, rb)
    if op in _LOGICAL:
        if dt is not None and dt != D.DT_BOOL:
            raise core.InvalidTypeException(f"{what}: '&' and '|' need boolean expressions, got {_type_name(dt)} "
                                            f"(put comparisons in parentheses)")
        return dt, rank
    if dt == D.DT_BOOL and op not in ("eq", "ne"):
        raise core.InvalidTypeException(f"{what}: arithmetic or ordering on boolean expressions; cast them first")
    if op in _COMPARE:
        return (D.DT_BOOL if dt is not None else None), rank
    if op == "div" and dt is not None and D.as_dtype(dt).is_integer:
        return D.DT_DOUBLE, rank  # integer '/' is a true division, in double
    return dt, rank


# ------------------------------------------------------------------ compilation
def _literal_for(v, dt: int):
    """A Python scalar is lifted by the graph builder with the tensor's dtype;
    an array literal is converted here."""
    if isinstance(v, np.ndarray):
        return np.asarray(v, dtype=D.numpy_dtype(dt))
    return v.item() if isinstance(v, np.generic) else v


def _expand(t, rank: int, to: int):
    from ..graph import dsl as tf
    for _ in range(to - rank):
        t = tf.expand_dims(t, -1)
    return t


def _build(e: tuple, df, phs: Dict[str, Any]):
    """DSL tensor of expression e over blocks of `df` -> (tensor, dtype, cell rank)."""
    from .. import core
    from ..graph import dsl as tf
    k = e[0]
    if k == "ref":
        name = e[1]
        dt, r = _field_info(df.schema, name)
        if name not in phs:
            phs[name] = core.block(df, name, tf_name=f"tfa_col_in_{len(phs)}")
        return phs[name], dt, r
    if k == "cast":
        t, _, r = _build(e[1], df, phs)
        return tf.cast(t, D.DType(e[2])), e[2], r
    if k == "un":
        t, dt, r = _build(e[2], df, phs)
        return (tf.negative(t) if e[1] == "neg" else tf.logical_not(t)), dt, r
    if k == "red":
        t, dt, r = _build(e[2], df, phs)
        if r == 0:
            return t, dt, 0
        fn = {"sum": tf.reduce_sum, "min": tf.reduce_min, "max": tf.reduce_max, "mean": tf.reduce_mean,
              "all": tf.reduce_all, "any": tf.reduce_any}[e[1]]
        return fn(t, list(range(1, r + 1))), dt, 0
    op, a, b = e[1], e[2], e[3]
    if a[0] == "lit":
        y, dt, rank = _build(b, df, phs)
        x = _literal_for(a[1], dt)
    elif b[0] == "lit":
        x, dt, rank = _build(a, df, phs)
        y = _literal_for(b[1], dt)
    else:
        x, dt, ra = _build(a, df, phs)
        y, _, rb = _build(b, df, phs)
        rank = max(ra, rb)
        x, y = _expand(x, ra, rank), _expand(y, rb, rank)
    fn = {"add": tf.add, "sub": tf.subtract, "mul": tf.multiply, "div": tf.truediv, "eq": tf.equal,
          "ne": tf.not_equal, "lt": tf.less, "le": tf.less_equal, "gt": tf.greater, "ge": tf.greater_equal,
          "and": tf.logical_and, "or": tf.logical_or}[op]
    out = fn(x, y)
    if op in _COMPARE:
        dt = D.DT_BOOL
    elif op == "div" and D.as_dtype(dt).is_integer:
        dt = D.DT_DOUBLE
    return out, dt, rank


def compile_expressions(df, exprs: Sequence[Tuple[str, tuple]]):
    """One graph computing every (node name, expression) over blocks of `df`.
    Returns (fetch tensors, {placeholder name: column}, [(dtype, cell rank)]).
    Types are checked against the frame's schema first (typed errors, before
    anything is built)."""
    from ..graph import dsl as tf
    infos = [_typeof(e, df.schema) for _, e in exprs]
    g = tf.Graph()
    phs: Dict[str, Any] = {}
    outs = []
    with g.as_default():
        for (node_name, e), _ in zip(exprs, infos):
            t, _, _ = _build(e, df, phs)
            outs.append(tf.identity(t, name=node_name))
    feed = {ph.op.name: cname for cname, ph in phs.items()}
    return outs, feed, infos
