"""The class rules of the multilevel hierarchy (csrc/pgo_ml_plan.hip: ml_plan) restated in Python, and the graph shapes whose class the
tests assert: test_pgo_hierarchy_gpu.py on the device's hierarchy, test_ml_plan.py on the plan alone (no GPU)."""

LDS_LIMIT = 140 * 1024          # kMlLdsLimit
MAX_PARTIALS = 8192             # kMaxPartials: workgroups of ml_spmv
MAX_LEVELS = 8                  # kMlMaxLevels
CHAIN = 6 * 48 + 3              # kChain (pgo_ml_kernels.hip): LDS doubles per ancestor level of the walked hierarchy


def levels1(nb):
    """ml_plan, agg = 1: levels of 8 until <= 8 aggregates remain, <= kMlTopWide = 16 above the dense level 1."""
    n = [nb, -(-nb // 8)]
    if n[1] > 8:
        n.append(-(-n[1] // 8))
        while n[-1] > 16:
            n.append(-(-n[-1] // 8))
    return n


def levels4(nb, dense=True):
    """ml_plan, agg = 4: fans 8, 4, 8, ..; <= 16 aggregates at the top above the dense level 2 (dense: comp4 not switched off and
    6 n_2 <= 18432), <= 8 when the PCG kernels walk the hierarchy."""
    n = [nb, -(-nb // 8)]
    n.append(-(-n[-1] // 4))
    if n[2] > 8:
        n.append(-(-n[2] // 8))
        while n[-1] > (16 if dense else 8):
            n.append(-(-n[-1] // 8))
    return n


# (free vertices, edges): 65 the first with two levels; C1; 1024 / 1025: n_2 = 16, the 96-row top level, against 17, which adds a level;
# C2 and 1281: 6 n_1 = 750 / 966 (<= kGemm32Max: ml_ns_gemm32); 2049 and 3072: the general GEMM, 6 n_1 = 1542 / 2304
DENSE1 = [(65, 200), (99, 300), (513, 2000), (1024, 4000), (1025, 4000), (999, 5000), (1281, 5000), (2049, 8000), (3072, 12400)]


def spmv_groups(nb, agg):
    """g_ml_spmv: AGG = 4 runs two half workgroups per 32-row level-2 aggregate."""
    return -(-nb // 8) if agg == 1 else 2 * -(-nb // 32)


def cg_lds_bytes(n, agg):
    """ml_cg_lds_bytes: what the walked hierarchy stages - every level from the gather level up, the offsets of those below the top, the
    top inverse's rows and a chain per ancestor level."""
    L = len(n) - 1
    g = 1 if (agg == 1 or L < 2) else 2
    d = sum(6 * n[l] for l in range(g, L + 1)) + sum(3 * n[l] for l in range(g, L))
    d += (agg * 6 if L == 1 else 6) * 6 * n[L]
    if L > 2:
        d += (L - 2) * CHAIN
    return 8 * d


def expected_class(nb, nslots, precond_on=True, strong_blocks=False, mult_banned=False, comp4_off=False):
    """The rules, one by one; block-Jacobi is dict(levels=0)."""
    if nb <= 8 or not precond_on:
        return dict(levels=0)
    loopy = nslots >= 6 * nb
    agg = 1 if (nb <= (3072 if loopy else 4096) and not strong_blocks) else 4
    if agg == 1:
        n = levels1(nb)
        cl = 1 if (len(n) - 1 >= 2 and 6 * n[1] <= 3072) else 0
        assert cl == 1 or len(n) == 2                       # (agg = 1 means nb <= 4096: 6 n_1 <= 3072 always holds)
    else:
        dense = not comp4_off and 6 * -(-(-(-nb // 8)) // 4) <= 18432
        n = levels4(nb, dense)
        cl = 2 if (dense and len(n) - 1 >= 3) else 0
    L = len(n) - 1
    assert L <= MAX_LEVELS
    lds = 48 * n[2] + 64 if cl == 2 else cg_lds_bytes(n, agg)
    if lds > LDS_LIMIT or spmv_groups(nb, agg) > MAX_PARTIALS:
        return dict(levels=0)
    mult = 1 if (cl > 0 and not mult_banned) else 0
    return dict(levels=L, agg=agg, cl=cl, gather_level=1 if (agg == 1 or L < 2) else 2, mult=mult,
                ns_steps=(4 if (agg == 4 and loopy) else 2) if mult else 0, lds=lds, n=n,
                fan=[1] + [4 if (l == 2 and agg == 4) else 8 for l in range(1, L + 1)])
