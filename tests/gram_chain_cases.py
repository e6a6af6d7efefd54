"""The inputs of tests/test_gpu_gram_chain.py and what each of them is expected to launch: the kernels of the UNFUSED Gram chain -- the
stand-alone Gram kernels behind the plain sweep (k_gram_small<1 ... 8>, k_gram<1 ... 4>, k_gram_block in every instantiation of
launch_gram), the three assembling kernels (k_gather_sum, k_assemble_sparse, k_assemble) and the two finishes of a J^T v product
(k_jtv_finish, the three-launch chain) -- at the sizes where each of them is the one that runs.  The models, the data and the layout
rules are those of tests/gram_layout_cases.py (Case, expK, form_active, expect); tests/test_cpu_gram_chain_cases.py checks, without a
GPU, that the oracle is a sound reference on every new input, that the expectations below cover what this text claims, and that
every new translation unit compiles.

THE DISPATCH RULES of the chain are restated here from the sources -- gram.hip: launch_gram (which Gram instantiation, which
blocks), launch.cpp: launch_gram_chain and packed_layout.cpp: build_gather_lists (source lists for k_gather_sum up to 2^18 entries of the packed
image, else k_assemble_sparse or k_assemble), passes.cpp: sweep_pass (the tail) and jtv_finish (one launch up to 4096 per-dataset
entries) -- and the GPU tests hold Context.debug_chain(), which reports what the host launched, against expect_chain().

Part E: beyond the fused kernel at every block shape: one dataset of expK(120), 145 ... 193 active (T = 10, 11, 13).
Part F: the stand-alone Gram under GADFIT_HIP_FUSED=0: Part A's counts, layout B1 of every form, 33 active and T = 7, 1 ... 8 active, layout B2.
Part G: 512 and 513 datasets of expK(4): the single-launch finish at its limit and past it, the dense image past 2^18 entries.
Part H: 48 and 49 datasets of the 128-parameter form: the pattern-only image on either side of 2^18 entries."""
from tests import gram_layout_cases as GL
from tests.gram_layout_cases import Case

GATHER_MAX = 1 << 18          # packed_layout.cpp: build_gather_lists, n_img <= 1 << 18
JTV_FINISH_MAX = 4096         # passes.cpp: jtv_finish, n_datasets * na <= 4096 (jtv.hip: k_jtv_finish, V[4096])


# ---- the dispatch rules of the chain ----------------------------------------------------------------------------------------------
def gram_launches(na):
    """gram.hip: launch_gram, in launch order"""
    if na <= 8:
        return ['small<%d>' % na]
    T = GL.tiles(na)
    if T <= 4:
        return ['gram<%d>' % T]
    if T <= 6:
        return ['block<%d,%d,true>@(0,0)' % (T, T)]
    out = []
    for gi in range(0, T, 4):
        for gj in range(gi, T, 4):
            tr, tc = min(4, T - gi), min(4, T - gj)
            out.append('block<%d,%d,true>@(%d,%d)' % (tr, tr, gi, gj) if gi == gj else 'block<4,%d,false>@(%d,%d)' % (tc, gi, gj))
    return out


def image_entries(c, sparse_ok=True):
    """doubles of the packed image [J^T J or its pattern | J^T r | chi2] (packed_layout.h: PackedLayout::packed_n)"""
    if GL.pattern_only(c.nd, c.active, c.is_global, sparse_ok):
        return GL.pattern_nnz(c.nd, c.active, c.is_global) + c.dim + 1
    return c.dim * c.dim + c.dim + 1


def expect_chain(c, tail_on=True, sparse_ok=True, fused_on=True, merge_small=True):
    """what Context.debug_chain() reports after a sweep and a J^T v product of this case on one rank"""
    lay = c.expect(tail_on=tail_on, sparse_ok=sparse_ok, fused_on=fused_on)
    if lay['tail_mode']:
        assemble = 'tail'
    elif c.nd * partial_stride(GL.tiles(c.na)) < 1 << 31 and image_entries(c, sparse_ok) <= GATHER_MAX:
        assemble = 'k_gather_sum'
    else:
        assemble = 'k_assemble_sparse' if lay['sparse'] else 'k_assemble'
    return dict(gram=[] if lay['fused'] else gram_launches(c.na), assemble=assemble,
                jtv_finish='k_jtv_finish' if merge_small and c.nd * c.na <= JTV_FINISH_MAX else 'chain')


def partial_stride(T):
    """gram_image.h: gram_partial_stride"""
    return (T * (T + 1) // 2 * 256 + 16 * T + 1 + 3) & ~3


def chi2_is_bitwise(c, fused_on=True):
    """is chi2() at a sweep's parameters bitwise the sweep's sum of squares?  launch.cpp claims it for the fused kernel, for up to 8
    active parameters on the two-kernel path (k_gram_small) and for k_gram_block; k_gram<T> makes no such promise"""
    return (fused_on and c.fused) or c.na <= 8 or GL.tiles(c.na) > 4


# ---- Part E: beyond the fused kernel, every block shape ---------------------------------------------------------------------------
E_K = 120
E_COUNTS = (145, 160, 161, 176, 193)          # T = 10, 10, 11, 11, 13
E_POINTS = (65, 1025, 2049)                   # 1025: 1536 slots, an odd number of 512-passes


def part_e():
    return [Case('E-%d-n%d' % (na, n), 'E', 'exp', E_K, GL._not_a_prefix(2 * E_K + 1, na), [n]) for na in E_COUNTS for n in E_POINTS]


# ---- Part F: the stand-alone Gram under GADFIT_HIP_FUSED=0 ------------------------------------------------------------------------
F_B1_FORMS = (16, 32, 48, 80, 96, 128)
F_POINTS = (65, 1025, 2049)
F_T7 = (97, 111)                              # T = 7 through the block loop: one live row / one padding row in the last tile
F_T3 = (33,)                                  # k_gram<3> with one live row in its last tile (Part A goes from 17 to 49: no first count of T = 3)
F_SMALL_POINTS = (1, 1025, 2049)
F_B2_FORMS = (32, 96)


def f_a():
    return GL.part_a()


def f_b1():
    out = []
    for na in F_B1_FORMS:
        K, active, _ = GL.form_active(na)
        out += [Case('F-B1-%d-n%d' % (na, n), 'F', 'exp', K, active, [n]) for n in F_POINTS]
    return out


def f_t7():
    """one dataset of 1501 points and an active list with a gap, as Part A's expK cases"""
    return [Case('F-exp-%d' % na, 'F', 'exp', (na + 1) // 2 + 1, GL._not_a_prefix(2 * ((na + 1) // 2 + 1) + 1, na), [GL.A_POINTS]) for na in F_T3 + F_T7]


def f_small():
    return [Case('F-small-%d-n%d' % (na, n), 'F', 'exp', (na + 1) // 2, list(range(na)), [n]) for na in range(1, 9) for n in F_SMALL_POINTS]


def f_b2():
    return [GL.b2(na) for na in F_B2_FORMS]


def part_f():
    return f_a() + f_b1() + f_t7() + f_small() + f_b2()


# ---- Part G: many datasets --------------------------------------------------------------------------------------------------------
G_K = 4
G_DATASETS = (512, 513)
G_SIZES = (1, 2, 3, 65)


def part_g_case(nd):
    """expK(4), parameters 0 ... 7 active, all of them global but the first amplitude"""
    return Case('G-%d' % nd, 'G', 'exp', G_K, list(range(8)), [G_SIZES[d % 4] for d in range(nd)], [0] + [1] * 7 + [0])


def part_g():
    return [part_g_case(nd) for nd in G_DATASETS]


# ---- Part H: the pattern-only image on either side of 2^18 entries -----------------------------------------------------------------
H_FORM = 128
H_DATASETS = (48, 49)


def part_h_case(nd):
    K, active, glob = GL.form_active(H_FORM)
    return Case('H-%d' % nd, 'H', 'exp', K, active, [3 + (19 * d) % 58 for d in range(nd)], glob)


def part_h():
    return [part_h_case(nd) for nd in H_DATASETS]


def new_inputs():
    """the cases whose data or active list no case of tests/gram_layout_cases.py has (the oracle is shown sound on those there)"""
    return part_e() + [c for c in f_b1() if c.sizes == [1025]] + f_t7() + f_small() + part_g() + part_h()


def all_cases():
    return part_e() + part_f() + part_g() + part_h()


def units():
    """[(tape, active list, n_datasets, store the Jacobian?)]: the translation units these parts ask for beyond those of
    tests/gram_layout_cases.py: units() -- every case here runs with the Jacobian store (the two-kernel path re-reads J; parts G and
    H keep the default)"""
    have = set((id(t), tuple(a), n * t.n_pars if n * t.n_pars <= GL.KERNARG_MAX else 0, bool(s)) for t, a, n, s in GL.units())
    out = []
    for c in all_cases():
        key = (id(c.tape()), tuple(c.active), c.kernarg, True)
        if key not in have:
            have.add(key)
            out.append((c.tape(), c.active, c.nd, True))
    return out
