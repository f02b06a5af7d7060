"""The table "Environment switches" of DESIGN.md section 6 is the index of every NEP_* variable the package reads: this test
keeps the two equal, keeps the retired switches retired, and keeps the "set by test" column true.  Host only: it reads sources."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nonlineareigenproblems.jl_amd")
NAME = r"NEP_[A-Z0-9_]+"

# the switches removed with the introduction of the table; none of them may come back under the same name
RETIRED = set("""
NEP_WEP_DFT_XCD NEP_WEP_DFT_RB NEP_WEP_DFT_COLS NEP_WEP_PINV_SYM NEP_WEP_SMW_BATCH NEP_SPMM_XCD NEP_K2_CM_ORDER NEP_K2_SP_GRID
NEP_K2_SP_CM_KMIN NEP_K2_TILE_KMAX NEP_K1_TILE_KMIN NEP_K1_TILE_KMAX NEP_K1_TILE_SMALL_KMIN NEP_K1_TILE_THREADS NEP_K1_TILE_NCU
NEP_K1_MODE NEP_NO_SHIFT_FOLD NEP_GEMM_RES NEP_DOTS_TARGET NEP_ORTH_NT NEP_ORTH_NT_MB NEP_ORTH_NT_FULL_MB NEP_ORTH_NPART
NEP_ML_INV_2STREAM NEP_ML_FUSE_MODE NEP_LU_PLAN_GPU NEP_LU_BATCH_BUILD NEP_LU_WIDE_MAXBLK NEP_IAR_RESID_OVERLAP NEP_IAR_NO_MIRROR
NEP_IAR_POLL_LAST NEP_IAR_EIG_CANDIDATES NEP_IAR_EIG_PROBE NEP_IAR_EIG_PRIO NEP_IAR_CHECK_PRIO NEP_IAR_EIG_MSSTEP NEP_IAR_BATCH
NEP_IAR_RECORD_ALL NEP_WEP_SMW_INV NEP_WEP_GRAPH NEP_WEP_GEMM NEP_TIAR_DEFER NEP_NO_ORDER_CACHE NEP_NLEIGS_SYNC
NEP_NLEIGS_BLAS_GUARD NEP_IAR_BLAS_GUARD NEP_LU_CACHE_BATCH NEP_GMRES_TRUE_RESIDUAL NEP_GMRES_SYNC NEP_EIG_ZGEEV
NEP_BEYN_SOLVE_STREAMS NEP_BEYN_BUILDERS NEP_BEYN_AHEAD NEP_ALIGNED_PREFETCH_NNZ NEP_IAR_POLL_US NEP_IAR_THROTTLE
NEP_IAR_CHECK_MAIN_STREAM
""".split())


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _package_sources():
    return sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))
                  + glob.glob(os.path.join(PKG, "*.py")) + glob.glob(os.path.join(PKG, "_workers", "*.py")))


def _reads(text):
    """names a source reads: arguments of getenv / nep_env_* (C++) and of the _env helpers / os.environ (Python), and names kept as
    whole string literals for such a call (a loop over names, a tuple of names)"""
    calls = re.findall(r"(?:getenv|nep_env_int|nep_env_double|nep_env_flag|env_int|env_float|env_flag|env_str|environ\.get|environ\.pop)"
                       r"\(\s*[\"'](" + NAME + r")[\"']", text)
    subscripts = re.findall(r"environ\[\s*[\"'](" + NAME + r")[\"']\s*\]", text)
    membership = re.findall(r"[\"'](" + NAME + r")[\"']\s+(?:not\s+)?in\s+os\.environ", text)
    literals = re.findall(r"[\"'](" + NAME + r")[\"']", text)
    return set(calls) | set(subscripts) | set(membership) | set(literals)


def _table():
    """variable -> "set by" cell of the section 6 table"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("### Environment switches")
    end = text.index("\n## ", start)
    rows = {}
    for line in text[start:end].splitlines():
        m = re.match(r"^\| `(" + NAME + r")` \|(.*)\|\s*$", line)
        if m:
            cells = [c.strip() for c in m.group(2).split("|")]
            assert len(cells) == 4, line                      # default, read, effect, set by
            assert cells[1] in ("process", "create", "call"), line
            assert m.group(1) not in rows, "listed twice: " + m.group(1)
            rows[m.group(1)] = cells[3]
    return rows


def test_table_lists_exactly_the_variables_the_package_reads():
    read = set()
    for path in _package_sources():
        read |= _reads(_read(path))
    bench_only = {v for v in _reads(_read(os.path.join(ROOT, "bench.py"))) if v.startswith("NEP_BENCH_") or v == "NEP_FORCE_DIST"}
    table = set(_table())
    assert len(read) > 50, read                               # the collection itself works
    assert read - table == set(), "read by the package, missing from the DESIGN.md table: %s" % sorted(read - table)
    assert table - read - bench_only == set(), "in the DESIGN.md table, read by nothing: %s" % sorted(table - read - bench_only)
    assert bench_only <= table, sorted(bench_only - table)


def test_retired_switches_stay_retired():
    assert len(RETIRED) == 57
    me = os.path.abspath(__file__)
    paths = _package_sources() + [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*"), recursive=True))
                                  if os.path.isfile(p) and os.path.abspath(p) != me and p.endswith((".py", ".sh", ".c", ".h", ".hip", ".md", ".txt", ".json"))]
    assert len(paths) > 40
    for path in paths:
        back = set(re.findall(NAME, _read(path))) & RETIRED
        assert not back, "%s names retired switches: %s" % (os.path.relpath(path, ROOT), sorted(back))


def test_rows_marked_test_are_named_by_a_test():
    named = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True):
        if os.path.abspath(path) != os.path.abspath(__file__):
            named |= set(re.findall(NAME, _read(path)))
    marked = [v for v, who in _table().items() if "test" in [w.strip() for w in who.split(",")]]
    assert len(marked) > 30, marked
    missing = [v for v in marked if v not in named]
    assert not missing, "marked 'test' in the DESIGN.md table but named by no file under tests/: %s" % missing
