"""The argument rules of the C entry points, one table per entry (ctypes, lz.hip_lib()).

Every entry gets one valid call (LZ_OK) and one row per rule it has, with exactly one
argument made invalid: LZ_E_ARG and the message part of lz_last_error's text ("argument
error: <message> (<condition>)"; the parenthesised condition is not part of the contract).
A row that must move a second argument to keep a single fault says so.  Overlap rows put a
second buffer one element (8 bytes) inside the first; where the moved buffer must stay on
16 bytes (the panel, a solve's work) it is two elements.  The edge rows hold what an
overlap rule must NOT reject: buffers that touch, and the pointer-equality rules (B and W
of a first cycle, Z and X of a term step), which accept a partial overlap.

Shapes: the 5-point Laplacian of an 8 x 8 grid (n = 64; also P, p = 64, of the normal
form), b = 4, m = 3, r = 1, degree 2, fp64.  All device buffers are 256 KiB slots of one
allocation, wide enough for the spans of the b = 65 rows, so no row has a second fault.
Invalid calls return before any launch.
"""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, PR, NB_, M, R, DEG = 64, 64, 4, 3, 1, 2
ES = 8
NB = N * NB_             # elements of one block
VS = NB + 32             # the panel's stride: 32 elements of padding
SPAN = (M - 1) * VS + NB  # the panel is one span of this many elements
SLOT = 1 << 18           # bytes per buffer slot
LZ_OK, LZ_E_ARG = 0, -1

CYCLES = [f"lz_block_lanczos_reorth{res}{form}" for res in ("", "_resume") for form in ("", "_cheb", "_normal", "_series")]
ENTRIES = ["lz_cheb_apply", "lz_cheb_series_apply", "lz_normal_apply", *CYCLES, "lz_panel_apply", "lz_csr_spmm_axpby",
           "lz_csr_spmm_axpby_dots", "lz_csr_spmm_axpby4", "lz_cheb_moments", "lz_col_dots", "lz_cg_update",
           "lz_cg_solve", "lz_bcg_update", "lz_bcg_direction", "lz_bcg_solve", "lz_csr_transpose"]


class At:
    """`off` bytes past the valid call's argument `name`"""

    def __init__(self, name, off):
        self.name, self.off = name, off


def nulls(names, msg):
    return [({k: None}, msg) for k in names.split()]


def inside(second, first, msg, off=ES):
    return ({second: At(first, off)}, msg)


def pairwise(names, msg):
    return [inside(c, a, msg) for a, c in itertools.combinations(names.split(), 2)]


CSR_ROWS = [({"nnz": -1}, "negative size"), ({"rp": None}, "row_ptr is NULL"), ({"col": None}, "col/val NULL"),
            ({"val": None}, "col/val NULL")]
DTYPE_ROW = [({"dtype": 7}, "dtype")]


def shape_rows(msg, bmax):
    return [({"n": 0}, msg), ({"b": bmax + 1}, msg)]


class Env:
    """The buffers of the valid calls, and what must outlive the calls that point to it."""

    def __init__(self, lz, handle, torch):
        self.lz, self.keep = lz, []
        rng = np.random.default_rng(77)
        self.names = {}
        self.arena = torch.from_numpy(rng.uniform(-1, 1, 48 * SLOT // 8)).cuda()
        self.A = lz.CsrDevice.from_host(lz.gen_laplace2d(8, 8))
        self.At = self.A.transpose(handle)
        assert self.A.n == N and self.At.n == N

    def slot(self, name):
        i = self.names.setdefault(name, len(self.names))
        assert (i + 1) * SLOT <= self.arena.numel() * 8
        return self.arena.data_ptr() + i * SLOT

    def host(self, obj):
        self.keep.append(obj)
        return ctypes.addressof(obj)

    def cheb(self, degree=DEG, lo=0.0, hi=6.0, ref=8.0):
        return self.host(self.lz.ChebFilter(degree, lo, hi, ref))

    def opts(self, tol=1e-8, max_iter=2, check_every=0, max_restarts=0):
        return self.host(self.lz.CgOpts(tol, max_iter, check_every, max_restarts))

    def csr(self, A=None, pre=""):
        A = A or self.A
        return {pre + "rp": A.row_ptr.data_ptr(), pre + "col": A.col.data_ptr(), pre + "val": A.val.data_ptr()}


def apply_table(env, name):
    """lz_cheb_apply, lz_cheb_series_apply, lz_normal_apply"""
    s = env.slot
    base = dict(n=N, nnz=env.A.nnz, **env.csr(), dtype=env.lz.LZ_F64, b=NB_, X=s("X"), Y=s("Y"), work=s("work"))
    apart = "X, Y and work must be pairwise distinct"
    rows = CSR_ROWS + DTYPE_ROW + pairwise("X Y work", apart)
    if name == "lz_cheb_apply":
        names = "n nnz rp col val dtype b f X Y work"
        base.update(f=env.cheb())
        rows += shape_rows("n >= 1, b in [1,64]", 64) + nulls("f X Y work", "f/X/Y/work NULL")
        rows += [({"f": env.cheb(degree=0)}, "Chebyshev filter: 1 <= degree <= 256"),
                 ({"f": env.cheb(degree=257)}, "Chebyshev filter: 1 <= degree <= 256"),
                 ({"f": env.cheb(lo=6.0)}, "Chebyshev filter: lo < hi, finite"),
                 ({"f": env.cheb(hi=float("inf"))}, "Chebyshev filter: lo < hi, finite"),
                 ({"f": env.cheb(ref=3.0)}, "Chebyshev filter: ref outside [lo, hi]")]
    elif name == "lz_cheb_series_apply":
        names = "n nnz rp col val dtype b degree lo hi gamma X Y work"
        base.update(degree=DEG, lo=0.0, hi=8.0, gamma=env.host((ctypes.c_double * (DEG + 1))(0.5, 0.25, 0.125)))
        rows += shape_rows("n >= 1, b in [1,64]", 64) + nulls("X Y work", "X/Y/work NULL") + series_rows()
    else:
        names = "n p nnz rp col val t_rp t_col t_val dtype b X Y work"
        base.update(p=PR, **env.csr(env.At, "t_"))
        shape = "n, p >= 1, b in [1,64]"
        rows += shape_rows(shape, 64) + [({"p": 0}, shape)] + nulls("X Y work", "X/Y/work NULL")
        rows += [({"t_rp": None}, "row_ptr is NULL"), ({"t_col": None}, "col/val NULL"), ({"t_val": None}, "col/val NULL")]
    # touching buffers: Y right behind X, work right behind Y
    rows += [({"Y": At("X", NB * ES)}, None), ({"work": At("Y", NB * ES)}, None)]
    return names, base, rows


def series_rows():
    return [({"degree": 0}, "Chebyshev series: 1 <= degree <= 65536"),
            ({"degree": 65537}, "Chebyshev series: 1 <= degree <= 65536"),
            ({"lo": 8.0}, "Chebyshev series: lo < hi, finite"), ({"hi": float("nan")}, "Chebyshev series: lo < hi, finite"),
            ({"gamma": None}, "Chebyshev series: gamma is NULL")]


def cycle_table(env, name):
    """the four lz_block_lanczos_reorth* and the four lz_block_lanczos_reorth_resume*"""
    s = env.slot
    resume = "_resume" in name
    form = name.rsplit("_", 1)[1] if name.rsplit("_", 1)[1] in ("cheb", "normal", "series") else "plain"
    head = "n p nnz rp col val t_rp t_col t_val dtype b" if form == "normal" else "n nnz rp col val dtype b"
    mid = "r m lc sigma" if resume else "m lc B"
    tail = {"plain": "", "cheb": "f work", "normal": "work", "series": "degree lo hi gamma work"}[form]
    names = f"{head} {mid} q alpha beta V vstride W passes {tail}"
    base = dict(n=N, nnz=env.A.nnz, **env.csr(), dtype=env.lz.LZ_F64, b=NB_, r=R, m=M, lc=5, sigma=s("sigma"), B=s("B"),
                q=s("q"), alpha=s("alpha"), beta=s("beta"), V=s("V"), vstride=VS, W=s("W"), passes=2, work=s("work"))
    rows = CSR_ROWS + DTYPE_ROW
    rows += [({"n": 0}, "n >= 1"),  # (lc is then no row index either: the n rule comes first)
             ({"b": 33, "vstride": N * 33}, "a basis panel supports 1 <= b <= 32"),  # (vstride follows b)
             ({"m": 65}, "the kept basis holds 1 <= m <= 64 blocks"),
             ({"V": None}, "V is NULL"), ({"vstride": NB - 2}, "vstride >= n*b"),
             ({"vstride": VS + 1}, "V and vstride must be multiples of 16 bytes"),
             ({"V": At("V", 8)}, "V and vstride must be multiples of 16 bytes"),
             ({"passes": 3}, "passes in {0, 1, 2}"), ({"passes": -1}, "passes in {0, 1, 2}"),
             ({"lc": -1}, "lc must be a row index"), ({"lc": N}, "lc must be a row index")]
    others = "W"  # what work must be apart from, beside the panel
    if resume:
        apart = "W and the panel V must be distinct buffers"
        keeps = "a resumed solve keeps 1 <= r < m blocks"
        rows += [({"r": 0}, keeps), ({"r": M}, keeps), ({"sigma": None}, "sigma is NULL")]
        rows += nulls("q alpha beta W", "NULL buffer")
    else:
        apart = "B, W and the panel V must be distinct buffers"
        others = "W B"
        rows += [({"m": 0}, "the kept basis holds 1 <= m <= 64 blocks")] + nulls("B q alpha beta W", "NULL buffer")
        rows += [inside("B", "V", apart), ({"V": At("B", 16)}, apart), ({"B": At("W", 0)}, apart),
                 ({"B": At("W", ES)}, None)]  # B == W is the rule: a partial overlap is accepted
    rows += [inside("W", "V", apart), ({"V": At("W", 16)}, apart),
             ({"W": At("V", SPAN * ES)}, None),                      # W right behind the panel's span
             ({"W": At("V", (SPAN - 1) * ES)}, apart),               # ... and one element into its last block
             ({"vstride": 3 * NB, "W": At("V", NB * ES)}, apart)]    # W in the padding: the panel is one span
    if form == "cheb":
        base.update(f=env.cheb())
        rows += [({"f": env.cheb(degree=0)}, "Chebyshev filter: 1 <= degree <= 256"),
                 ({"f": env.cheb(degree=257)}, "Chebyshev filter: 1 <= degree <= 256"),
                 ({"f": env.cheb(lo=float("nan"))}, "Chebyshev filter: lo < hi, finite"),
                 ({"f": env.cheb(hi=0.0)}, "Chebyshev filter: lo < hi, finite"),
                 ({"f": env.cheb(ref=6.0)}, "Chebyshev filter: ref outside [lo, hi]"),
                 ({"f": None, "work": None}, None)]  # no filter: the plain operator, work unused
    elif form == "normal":
        base.update(p=PR, **env.csr(env.At, "t_"))
        rows += [({"p": 0}, "normal operator: p >= 1"),
                 ({"t_rp": None}, "normal operator: the transpose's row_ptr is NULL"),
                 ({"t_col": None}, "normal operator: the transpose's col/val NULL"),
                 ({"t_val": None}, "normal operator: the transpose's col/val NULL")]
    elif form == "series":
        base.update(degree=DEG, lo=0.0, hi=8.0, gamma=env.host((ctypes.c_double * (DEG + 1))(0.5, 0.25, 0.125)))
        rows += series_rows()
    if form != "plain":
        apart = "work must not overlap B, W or the panel V"
        rows += [({"work": None}, "work is NULL"), ({"work": At("work", 8)}, "work must be on 16 bytes")]
        for o in others.split():
            rows += [({"work": At(o, 16)}, apart), inside(o, "work", apart),
                     ({"work": At(o, NB * ES)}, None)]  # work right behind W (B), in one allocation
        rows += [({"work": At("V", 16)}, apart), ({"V": At("work", 16)}, apart),
                 ({"work": At("V", (SPAN - 2) * ES)}, apart), ({"work": At("V", SPAN * ES)}, None),
                 ({"vstride": 3 * NB, "work": At("V", NB * ES)}, apart)]
    return names, base, rows


def other_table(env, name):
    s, f64 = env.slot, env.lz.LZ_F64
    csr = dict(n=N, nnz=env.A.nnz, **env.csr(), dtype=f64, b=NB_)
    if name == "lz_panel_apply":
        names = "n b k dtype beta alpha V vstride S W"
        base = dict(n=N, b=NB_, k=M, dtype=f64, beta=1.0, alpha=-1.0, V=s("V"), vstride=VS, S=s("sigma"), W=s("W"))
        apart, blocks = "W must not overlap the panel", "a basis panel holds 1 <= k <= 64 blocks"
        rows = DTYPE_ROW + [({"n": 0}, "n >= 1"), ({"b": 33, "vstride": N * 33}, "a basis panel supports 1 <= b <= 32"),
                            ({"k": 0}, blocks), ({"k": 65}, blocks), ({"V": None}, "V is NULL"),
                            ({"vstride": NB - 2}, "vstride >= n*b"),
                            ({"vstride": VS + 1}, "V and vstride must be multiples of 16 bytes"),
                            ({"V": At("V", 8)}, "V and vstride must be multiples of 16 bytes")]
        rows += nulls("S W", "S/W NULL")
        rows += [inside("W", "V", apart), ({"V": At("W", 16)}, apart), ({"W": At("V", SPAN * ES)}, None),
                 ({"W": At("V", (SPAN - 1) * ES)}, apart), ({"vstride": 3 * NB, "W": At("V", NB * ES)}, apart)]
    elif name.startswith("lz_csr_spmm_axpby"):
        dots, four = name.endswith("_dots"), name.endswith("4")
        names = "n nnz rp col val dtype b a X c d Z" + (" e U" if four else "") + " Y" + (" dots" if dots else "")
        base = dict(csr, a=1.0, X=s("X"), c=0.5, d=-1.0, Z=s("Z"), e=0.25, U=s("U"), Y=s("Y"), dots=s("dots"))
        apart = "Y must be distinct from X, Z and U, and Z from X (no in-place form)"
        shape = "b in [1,64] (and n >= 1 with dots)"
        rows = CSR_ROWS + DTYPE_ROW + [({"b": 65}, shape)] + nulls("X Y Z", "X/Y NULL, or Z NULL with d != 0")
        rows += [inside("Y", "X", apart), inside("X", "Y", apart), inside("Y", "Z", apart), inside("Z", "Y", apart),
                 ({"Z": At("X", 0)}, apart),
                 ({"Z": At("X", ES)}, None),          # Z == X is the rule: a partial overlap is accepted
                 ({"Y": At("X", NB * ES)}, None),     # touching
                 ({"Z": None, "d": 0.0}, None)]       # no third term: Z unused
        if dots:
            rows += [({"n": 0}, shape), ({"dots": None}, "dots is NULL")]
        else:
            rows += [({"n": 0}, None)]  # no rows, nothing to do: accepted without dots
        if four:
            rows += [({"U": None}, "U NULL with e != 0"), inside("Y", "U", apart), inside("U", "Y", apart),
                     ({"U": None, "e": 0.0}, None), ({"U": At("X", 0)}, None)]  # U = X is the Clenshaw step's own use
    elif name == "lz_cheb_moments":
        names = "n nnz rp col val dtype b lo hi K X0 work dots"
        base = dict(csr, lo=0.0, hi=8.0, K=2, X0=s("X"), work=s("work"), dots=s("dots"))
        apart = "X0 and work must be distinct"
        rows = CSR_ROWS + DTYPE_ROW + shape_rows("n >= 1, b in [1,64]", 64) + nulls("X0 work dots", "X0/work/dots NULL")
        rows += [({"lo": 8.0}, "Chebyshev moments: lo < hi, finite"), ({"hi": float("inf")}, "Chebyshev moments: lo < hi, finite"),
                 ({"K": 0}, "Chebyshev moments: 1 <= K <= 65536"), ({"K": 65537}, "Chebyshev moments: 1 <= K <= 65536"),
                 inside("work", "X0", apart), inside("X0", "work", apart), ({"X0": At("work", (3 * NB - 1) * ES)}, apart),
                 ({"X0": At("work", 3 * NB * ES)}, None), ({"work": At("X0", NB * ES)}, None)]
    elif name == "lz_col_dots":
        names = "n b dtype Y X dots"
        base = dict(n=N, b=NB_, dtype=f64, Y=s("Y"), X=s("X"), dots=s("dots"))
        rows = DTYPE_ROW + shape_rows("n >= 1, b in [1,64]", 64) + nulls("Y X dots", "Y/X/dots NULL")
        rows += [({"Y": At("X", 0)}, None)]  # the dots of a block with itself
    elif name == "lz_cg_update":
        names = "n b dtype coef R W P S X rr"
        base = dict(n=N, b=NB_, dtype=f64, coef=s("coef"), R=s("R"), W=s("W"), P=s("P"), S=s("S"), X=s("X"), rr=s("rr"))
        rows = DTYPE_ROW + shape_rows("n >= 1, b in [1,64]", 64) + nulls("coef R W P S X rr", "coef/R/W/P/S/X/rr NULL")
        rows += pairwise("R W P S X", "R, W, P, S and X must be pairwise distinct")
        rows += [({"W": At("R", NB * ES)}, None)]
    elif name in ("lz_cg_solve", "lz_bcg_solve"):
        bmax = 64 if name == "lz_cg_solve" else 32
        names = "n nnz rp col val dtype b shift B X work opts iters status resid est info"
        base = dict(csr, shift=0.0, B=s("B"), X=s("X"), work=s("work"), opts=env.opts(),
                    iters=env.host((ctypes.c_int * 64)()), status=env.host((ctypes.c_int * 64)()),
                    resid=env.host((ctypes.c_double * 64)()), est=env.host((ctypes.c_double * 64)()),
                    info=env.host((ctypes.c_int * 8)()))
        apart, tol, its = "B, X and work must be pairwise distinct", "tol > 0, tol and shift finite", "max_iter, max_restarts >= 0"
        rows = CSR_ROWS + DTYPE_ROW + shape_rows(f"n >= 1, b in [1,{bmax}]", bmax)
        rows += nulls("B X work opts iters status resid est info", "NULL argument")
        rows += [({"opts": env.opts(tol=0.0)}, tol), ({"opts": env.opts(tol=float("inf"))}, tol), ({"shift": float("nan")}, tol),
                 ({"opts": env.opts(max_iter=-1)}, its), ({"opts": env.opts(max_restarts=-1)}, its)]
        rows += pairwise("B X work", apart) + [({"B": At("work", (4 * NB - 1) * ES)}, apart),
                                               ({"B": At("work", 4 * NB * ES)}, None), ({"work": At("X", NB * ES)}, None)]
    elif name == "lz_bcg_update":
        names = "n b dtype xi E S W Q X G"
        base = dict(n=N, b=NB_, dtype=f64, xi=s("xi"), E=s("E"), S=s("S"), W=s("W"), Q=s("Q"), X=s("X"), G=s("G"))
        rows = DTYPE_ROW + shape_rows("n >= 1, b in [1,32]", 32) + nulls("xi E S W Q X G", "xi/E/S/W/Q/X/G NULL")
        rows += pairwise("S W Q X", "S, W, Q and X must be pairwise distinct") + [({"W": At("S", NB * ES)}, None)]
    elif name == "lz_bcg_direction":
        names = "n b dtype z zinv Q S"
        base = dict(n=N, b=NB_, dtype=f64, z=s("xi"), zinv=s("E"), Q=s("Q"), S=s("S"))
        rows = DTYPE_ROW + shape_rows("n >= 1, b in [1,32]", 32) + nulls("z zinv Q S", "z/zinv/Q/S NULL")
        rows += [inside("S", "Q", "Q and S must be distinct"), inside("Q", "S", "Q and S must be distinct"),
                 ({"S": At("Q", NB * ES)}, None)]
    else:
        assert name == "lz_csr_transpose"
        names = "n_rows n_cols nnz rp col val dtype t_rp t_col t_val"
        base = dict(n_rows=N, n_cols=N, nnz=env.A.nnz, **env.csr(), dtype=f64, t_rp=s("t_rp"), t_col=s("t_col"),
                    t_val=s("t_val"))
        apart = "the outputs must be distinct from each other and from the inputs"
        rows = CSR_ROWS + DTYPE_ROW
        rows += [({"n_rows": 1 << 31}, "n_rows < 2^31 (t_col holds source rows)"),
                 ({"n_cols": 1 << 31}, "0 <= n_cols < 2^31"), ({"n_cols": -1}, "0 <= n_cols < 2^31"),
                 ({"nnz": (1 << 32) - 1}, "nnz < 2^32 - 1"), ({"n_rows": 0}, "entries without rows")]
        rows += nulls("t_rp t_col t_val", "output NULL")
        size = {"rp": 8, "col": 4, "val": ES, "t_rp": 8, "t_col": 4}
        rows += [inside(o, i, apart, size[i]) for o in ("t_rp", "t_col", "t_val") for i in ("rp", "col", "val")]
        rows += [inside("t_col", "t_rp", apart, 8), inside("t_val", "t_rp", apart, 8), inside("t_val", "t_col", apart, 4)]
    return names, base, rows


@pytest.fixture(scope="module")
def env(lz, handle, torch_cuda):
    return Env(lz, handle, torch_cuda)


def test_table_covers_the_entries():
    assert len(ENTRIES) == len(set(ENTRIES)) == 23 and len(CYCLES) == 8


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_rules(lz, handle, torch_cuda, env, name):
    table = apply_table if name.endswith("_apply") and "panel" not in name else cycle_table if name in CYCLES else other_table
    names, base, rows = table(env, name)
    names = names.split()
    fn, L = getattr(handle.L, name), handle.L

    def call(over):
        a = dict(base)
        a.update({k: base[v.name] + v.off if isinstance(v, At) else v for k, v in over.items()})
        return fn(handle.ptr, *[a[k] for k in names])

    assert call({}) == LZ_OK, L.lz_last_error()
    bad = []
    for over, msg in rows:
        assert set(over) <= set(names), (name, over)
        rc = call(over)
        text = L.lz_last_error().decode(errors="replace") if rc != LZ_OK else ""
        what = {k: (f"{v.name}+{v.off}" if isinstance(v, At) else v) for k, v in over.items()}
        if msg is None:
            if rc != LZ_OK:
                bad.append(f"{what}: accepted today, got {rc}: {text}")
        elif rc != LZ_E_ARG or not text.startswith(f"argument error: {msg} ("):
            bad.append(f"{what}: expected LZ_E_ARG '{msg}', got {rc}: {text}")
    torch_cuda.cuda.synchronize()
    print(f"{name}: {len(rows)} rows")
    assert not bad, "\n".join(bad)
