"""The inputs of tests/test_gpu_gram_layouts.py and what each of them is expected to reach: the fused sweep + Gram kernel's matrix-core
forms (1 ... 4 tiles on the full stage, 5 on the half stage with one reduction image, 6 ... 8 cooperative, beyond 128 parameters the plain
sweep and blocked Gram) crossed with the layouts of the points (one dataset or several, one-point datasets, one workgroup or many,
in-kernel tail or launch chain, dense or pattern-only image, parameter block by value or by pointer, pseudo-ranks).
tests/test_cpu_gram_layout_cases.py checks, without a GPU, that the oracle is a sound reference on every case, that the expectations
below cover what this text claims, and that every translation unit compiles.  Everything here is deterministic and needs no GPU.

THE DISPATCH RULES are restated here from the sources -- data.cpp: build_layout (padding, gram blocks), passes.cpp: sweep_pass (small,
tail, pattern-only), launch.cpp (tail_one_workgroup_per_cu, tail mode), active.cpp (get_kernels: the parameter block by value up to
480 doubles), packed_layout.cpp (compute_layout: the pattern) and codegen.h (fused_waves_for and the LDS of a workgroup) -- and the GPU tests hold
Context.debug_layout() against expect(): a threshold that moves fails there instead of moving a case off the path it is here for.

Part A: one dataset of 1501 points at the first active count of every form and at one below every full tile.
Part B: layouts B1 ... B5 x forms.  Part C: layout B3 over 3 and 8 pseudo-ranks."""
import functools

import numpy as np

from gadfit_amd.ad import exp, trace_model
from tests import models as M

# ---- model expK: y = p[2K] + sum_k p[2k] exp(-x / p[2k+1]) ------------------------------------------------------------------------
# No term of it and none of its derivatives vanishes or changes sign on x > 0, so datasets of one or two points keep every column of
# the Jacobian in the normal range (gaussK's peaks are exact or subnormal zeros away from their centres).


def make_model_expK(K):
    def model(p, x):
        y = p[2 * K]
        for k in range(K):
            y = y + p[2 * k] * exp(-(x / p[2 * k + 1]))
        return y
    return model


def expK_truth(K):
    p = np.zeros(2 * K + 1)
    for k in range(K):
        p[2 * k] = 1.0 + 2.0 * ((7 * k) % K) / K
        p[2 * k + 1] = 40.0 ** ((k + 0.5) / K)
    p[2 * K] = 0.5
    return p


def expK_numpy(K):
    def f(p, x):
        y = np.full_like(x, p[2 * K])
        for k in range(K):
            y += p[2 * k] * np.exp(-x / p[2 * k + 1])
        return y
    return f


def expK_rows(K, p, x):
    """(f, df/dp [n][2K+1]) in numpy.longdouble from the closed form"""
    p = np.asarray(p, dtype=np.longdouble); x = np.asarray(x, dtype=np.longdouble)
    g = np.zeros((x.size, 2 * K + 1), dtype=np.longdouble)
    f = np.full(x.size, p[2 * K], dtype=np.longdouble)
    for k in range(K):
        a, tau = p[2 * k], p[2 * k + 1]
        e = np.exp(-x / tau)
        f += a * e
        g[:, 2 * k] = e
        g[:, 2 * k + 1] = a * e * x / (tau * tau)
    g[:, 2 * K] = 1
    return f, g


def gaussK_rows(K, p, x):
    """the same for tests/models.py: make_model_gaussK"""
    p = np.asarray(p, dtype=np.longdouble); x = np.asarray(x, dtype=np.longdouble)
    g = np.zeros((x.size, 4 * K), dtype=np.longdouble)
    f = np.zeros(x.size, dtype=np.longdouble)
    for k in range(K):
        A, mu, w, s = p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]
        d = x - mu
        e = np.exp(-(d / w) ** 2)
        lin = 1 + s * d
        f += A * e * lin
        g[:, 4 * k] = e * lin
        g[:, 4 * k + 1] = A * e * (2 * d / (w * w) * lin - s)
        g[:, 4 * k + 2] = A * e * lin * 2 * d * d / (w * w * w)
        g[:, 4 * k + 3] = A * e * d
    return f, g


# ---- the dispatch rules -----------------------------------------------------------------------------------------------------------
PAD_GRANULE = PASS_GRANULE = GRAM_TARGET = 512          # context.h: kPadGranule; data.cpp: kPassGranule, kGramTarget
VALU_GRAM_MAX, FUSED_MAX_NO_COOP, FUSED_MAX = 8, 80, 128      # codegen.h: kValuGramMax, kFusedMaxActiveNoCoop, kFusedMaxActive
KERNARG_MAX = 480                                      # active.cpp: kMaxKernargPars
SMALL_MAX = 65536                                      # passes.cpp: dim * dim * nd <= 65536
LDS_BYTES = 160 * 1024


def tiles(na):
    return (na + 15) // 16


def fused_coop(na):
    return na > FUSED_MAX_NO_COOP


def fused_half_stage(na):
    return na > 64


def fused_single_image(na):
    return not fused_coop(na) and na > 64


def fused_lds_bytes_for(na, fw):
    T = tiles(na); npair = T * (T + 1) // 2
    stage = (16 * T + 1) * (34 if fused_half_stage(na) else 66)
    img = npair * 256 + 16 * T + 1
    if fused_coop(na):
        return max(fw * stage, T * 64 + 8 + img) * 8
    if fused_single_image(na):
        return max(fw * stage, npair * 256 + fw * (T * 64 + 4) + img) * 8
    red = npair * 256 + T * 64 + 4
    return fw * max(stage, red) * 8 + img * 8 + 64


def fused_waves_for(na):
    fw = 4 if fused_coop(na) else 8
    while fw > 1 and fused_lds_bytes_for(na, fw) > LDS_BYTES:
        fw //= 2
    return fw


def fused_lds_bytes(na):
    fw = fused_waves_for(na)
    if na <= VALU_GRAM_MAX:
        return (fw + 1) * (na * (na + 1) // 2 + na + 1) * 8 + 273 * 8 + 64
    return fused_lds_bytes_for(na, fw)


def tail_one_workgroup_per_cu(na):
    return fused_lds_bytes(na) > 80 * 1024


def form_of(na):
    if na > FUSED_MAX:
        return 'unfused'
    if na <= VALU_GRAM_MAX:
        return 'valu'
    if fused_coop(na):
        return 'coop'
    return 'half' if fused_half_stage(na) else 'full'


def partition(n_total, nranks, rank):
    """gfh_partition (gadfit.F90:978-983): int(N / nranks) each, the remainder one each to the first ranks"""
    sizes = [int((1.0 / nranks) * n_total) for _ in range(nranks)]
    rest = n_total - sum(sizes)
    sizes = [s + (1 if i + 1 <= rest else 0) for i, s in enumerate(sizes)]
    return sum(sizes[:rank]), sizes[rank]


def local_sizes(sizes, nranks=1, rank=0):
    """points of every dataset that rank `rank` holds"""
    pos = np.concatenate([[0], np.cumsum(sizes)])
    b, n = partition(int(pos[-1]), nranks, rank)
    return [int(max(0, min(b + n, pos[d + 1]) - max(b, pos[d]))) for d in range(len(sizes))]


def block_layout(sizes):
    """(n_slots, gram blocks per dataset) of datasets with these many local points"""
    padded = [(n + PAD_GRANULE - 1) // PAD_GRANULE * PAD_GRANULE for n in sizes]
    n_slots = sum(padded)
    per = (n_slots + GRAM_TARGET - 1) // GRAM_TARGET
    per = max(PASS_GRANULE, (per + PASS_GRANULE - 1) // PASS_GRANULE * PASS_GRANULE)
    if n_slots <= 4 * PASS_GRANULE:
        per = max(per, n_slots)
    return n_slots, [(s + per - 1) // per for s in padded]


def jacobian_indices(nd, active, is_global):
    """gfh_jacobian_indices (gadfit.F90:618-628): (jac [nd][na], dim)"""
    na = len(active); shift = 0
    jac = np.zeros((nd, na), dtype=np.int32)
    for i in range(nd):
        for j in range(na):
            if is_global[active[j]]:
                jac[i, j] = j
                shift += i > 0
            else:
                jac[i, j] = j + i * na - shift
    return jac, nd * na - shift


def pattern_nnz(nd, active, is_global):
    """(row <= col) pairs of columns that some dataset couples (packed_layout.cpp: compute_layout)"""
    jac, dim = jacobian_indices(nd, active, is_global)
    keys = set()
    for d in range(nd):
        r, c = np.meshgrid(jac[d], jac[d], indexing='ij')
        m = r <= c
        keys.update((c[m].astype(np.int64) * dim + r[m]).tolist())
    return len(keys)


def pattern_only(nd, active, is_global, sparse_ok=True):
    """does the image travel as its pattern (packed_layout.cpp: compute_layout, transfer_sparse)?"""
    dim = jacobian_indices(nd, active, is_global)[1]
    if dim * dim * nd <= SMALL_MAX or not sparse_ok or nd < 2:
        return False
    return 4 * (pattern_nnz(nd, active, is_global) + dim + 1) < dim * dim + dim + 1


class Case:
    def __init__(self, cid, part, model, K, active, sizes, is_global=None, fit=None, images=1):
        self.id, self.part, self.model, self.K, self.active, self.sizes = cid, part, model, K, list(active), list(sizes)
        self.n_pars = 2 * K + 1 if model == 'exp' else 4 * K
        self.is_global = list(is_global) if is_global is not None else [0] * self.n_pars
        self.fit = fit                      # options of a fit against the oracle's, or None
        self.images = images                # images the oracle cuts its point sums into (ORACLE_SUM_TOL below)
        self.na, self.nd = len(self.active), len(self.sizes)
        assert self.active == sorted(set(self.active)) and self.active[-1] < self.n_pars

    @property
    def dim(self):
        return jacobian_indices(self.nd, self.active, self.is_global)[1]

    @property
    def small(self):
        return self.dim * self.dim * self.nd <= SMALL_MAX

    @property
    def fused(self):
        return self.na <= FUSED_MAX

    @property
    def kernarg(self):
        return self.nd * self.n_pars if self.nd * self.n_pars <= KERNARG_MAX else 0

    def tape(self):
        return tape_of(self.model, self.K)

    def rows(self, pars, x):
        return (expK_rows if self.model == 'exp' else gaussK_rows)(self.K, pars, x)

    def data(self):
        """(xs, ys, ws, start [nd][n_pars]): dataset d has the local parameters of the truth scaled by 1 + 0.1 d and its own noise;
        start = start_values(its truth), the global parameters at start_values(the first dataset's truth)"""
        return _data(self.model, self.K, tuple(self.sizes), tuple(self.is_global))

    def expect(self, nranks=1, rank=0, tail_on=True, sparse_ok=True, fused_on=True):
        """what Context.debug_layout() reports after a sweep of this case on rank `rank` of `nranks` pseudo-ranks (tail_on, sparse_ok,
        fused_on: GADFIT_HIP_TAIL, GADFIT_HIP_SPARSE, GADFIT_HIP_FUSED of the context; without the fused kernel there is no tail)"""
        n_slots, blocks = block_layout(local_sizes(self.sizes, nranks, rank))
        n_gb = sum(blocks)
        fused = fused_on and self.fused
        tail = tail_on and fused and n_gb > 0 and self.small and (tail_one_workgroup_per_cu(self.na) or n_gb <= 256)
        return dict(n_slots=n_slots, n_gb=n_gb, datasets_with_blocks=sum(b > 0 for b in blocks), fused=int(fused),
                    waves=fused_waves_for(self.na) if fused else 0, tail_mode=2 if tail else 0,
                    sparse=int(pattern_only(self.nd, self.active, self.is_global, sparse_ok)), kernarg=self.kernarg)

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def tape_of(model, K):
    return trace_model(make_model_expK(K), 2 * K + 1) if model == 'exp' else trace_model(M.make_model_gaussK(K), 4 * K)


@functools.lru_cache(maxsize=None)
def _data(model, K, sizes, is_global):
    truth = expK_truth(K) if model == 'exp' else M.gaussK_truth(K)
    fn = expK_numpy(K) if model == 'exp' else M.gaussK_numpy(K)
    hi = 60.0 if model == 'exp' else 100.0
    glob = np.array(is_global, dtype=bool)
    amp = np.zeros(truth.size, dtype=bool)
    amp[0::2 if model == 'exp' else 4] = True          # amplitudes (and expK's background): what differs between the datasets
    xs, ys, ws, start = [], [], [], []
    for d, n in enumerate(sizes):
        t = truth.copy()
        t[amp & ~glob] *= 1.0 + 0.1 * d
        x, y, s = M.make_single(fn, t, n, 0.0, hi, seed=M.SEED + 5 * d)
        xs.append(x); ys.append(y); ws.append(1.0 / s)
        st = M.start_values(t)
        st[glob] = M.start_values(truth)[glob]
        start.append(st)
    return xs, ys, ws, np.array(start)


# ---- Part A: the first count of every form and one below every full tile, one dataset of 1501 points ------------------------------
A_FIRST = (9, 17, 49, 65, 81, 113, 129)          # gaussK(ceil(NA / 4) + 1): the heavy AD body
A_BELOW = (15, 31, 47, 63, 79, 127)              # expK
A_POINTS = 1501                                  # (gaussK: no abscissa on a start centre, tests/test_gpu_parity.py: test_gram_tile_counts_vs_oracle)


def _not_a_prefix(n_pars, na):
    """parameters 0, 1, 2, then a gap in the middle, then the rest: the column map is not the identity"""
    return [0, 1, 2] + list(range(3 + n_pars - na, n_pars))


def part_a():
    out = []
    for na in A_FIRST:
        K = (na + 3) // 4 + 1
        out.append(Case('A-gauss-%d' % na, 'A', 'gauss', K, _not_a_prefix(4 * K, na), [A_POINTS]))
    for na in A_BELOW:
        K = (na + 1) // 2 + 1
        out.append(Case('A-exp-%d' % na, 'A', 'exp', K, _not_a_prefix(2 * K + 1, na), [A_POINTS]))
    return out


# ---- Part B: layouts x forms ------------------------------------------------------------------------------------------------------
# One (model, active list) per form serves B1 ... B4: K decay times of which n_glob are active -- they are the global parameters of B2
# and B3 -- and n_loc active amplitudes (the background among them).  The two numbers are chosen so that
#   B2 (3 datasets; 2 for 96, 128 and 130) has dim^2 nd <= 65536: the in-kernel tail serves it,
#   B3 (8 datasets) has dim^2 nd > 65536: launch chain, pattern-only image,
# and K so that nd (2K + 1) > 480 in B2 and B3: the parameter block goes by pointer there and by value in B1, so that B1 ... B4 of a form
# share two translation units (a by-value block of several datasets would be one more per number of datasets).
#        NA: (K, n_glob, n_loc)
FORMS = {16: (80, 5, 11), 32: (80, 16, 16), 48: (80, 24, 24), 80: (80, 47, 33), 96: (120, 48, 48), 128: (120, 76, 52), 130: (120, 80, 50)}
FORM_NAMES = {16: '1 tile', 32: '2 tiles, 8 waves', 48: '3 tiles, 4 waves', 80: 'half stage, one image', 96: 'cooperative', 128: 'cooperative',
              130: 'beyond the fused kernel'}
B1_SIZES = (1, 63, 64, 65, 512, 513, 2048, 2049, 16897)
B1_SIZES_UNFUSED = (65, 2049)
B2_SIZES = [1, 700, 65]
B2_SIZES_TWO = [1, 700]                          # 96, 128, 130 active: three datasets are past dim^2 nd <= 65536 whatever the split
B3_SIZES = [1, 1024, 333, 2049, 57, 513, 2, 64]
B4_SIZES = (131072, 131073)                      # 256 and 257 gram blocks
B5_SIZES = [1337, 911, 1501]
C_FORMS = (32, 96)
C_RANKS = (3, 8)


def _spread(n, K):
    """n of 0 ... K-1, evenly spread"""
    return [(k * K) // n for k in range(n)]


def form_active(na):
    """(K, active list, is_global): every active decay time is global in the layouts of several datasets, the rest is local"""
    K, n_glob, n_loc = FORMS[na]
    assert n_glob + n_loc == na
    glob = [2 * k + 1 for k in _spread(n_glob, K)]
    loc = [2 * k for k in _spread(n_loc - 1, K)] + [2 * K]
    is_global = [0] * (2 * K + 1)
    for g in glob:
        is_global[g] = 1
    return K, sorted(glob + loc), is_global


def b1(na, n):
    K, active, _ = form_active(na)
    return Case('B1-%d-n%d' % (na, n), 'B1', 'exp', K, active, [n])


def b2(na):
    K, active, glob = form_active(na)
    return Case('B2-%d' % na, 'B2', 'exp', K, active, B2_SIZES if na < 96 else B2_SIZES_TWO, glob)


def b3(na):
    K, active, glob = form_active(na)
    return Case('B3-%d' % na, 'B3', 'exp', K, active, B3_SIZES, glob)


# The oracle adds its points one after the other, as one image of the reference does; its J^T J then carries a rounding error of its own
# that grows with the number of points.  Against the same sums in numpy.longdouble (tests/test_cpu_gram_layout_cases.py) it is at most
# 4.3e-14 on J^T J up to 16897 points, but 2.4e-13 and 2.2e-13 at B4's 131072 and 131073 points (J^T r 7.4e-14): more than the 1e-13 the
# device is held to, and what a first run of B4 on the device showed to the digit.  A comparison at 1e-13 needs a reference good to
# half of that, so that the other half is the device's: ORACLE_SUM_TOL.  B4's point counts are what B4 is about, so its oracle is the
# reference on 64 images (n_images: each image adds its share, the shares are added: co_sum), whose error there is 1.9e-15.
ORACLE_SUM_TOL = 5e-14
B4_IMAGES = 64


def b4(n):
    K, active, _ = form_active(16)
    return Case('B4-16-n%d' % n, 'B4', 'exp', K, active, [n], images=B4_IMAGES)


B5_FIT = dict(lambda_=1.0, max_iter=4)


def b5(K):
    """gaussK(K), all 4K parameters active, the centres global, three datasets; pass check and a 4-iteration fit"""
    return Case('B5-gauss-%d' % (4 * K), 'B5', 'gauss', K, list(range(4 * K)), B5_SIZES, [1 if k % 4 == 1 else 0 for k in range(4 * K)], fit=B5_FIT)


def part_b():
    out = []
    for na in FORMS:
        out += [b1(na, n) for n in (B1_SIZES if na <= FUSED_MAX else B1_SIZES_UNFUSED)]
        out.append(b2(na))
        if na <= FUSED_MAX:
            out.append(b3(na))
    return out + [b4(n) for n in B4_SIZES] + [b5(24), b5(8)]


def part_c():
    """[(case, nranks)]: layout B3 on pseudo-ranks"""
    return [(b3(na), nranks) for na in C_FORMS for nranks in C_RANKS]


def all_cases():
    return part_a() + part_b()


def units():
    """[(tape, active list, n_datasets, store the Jacobian?)]: every distinct translation unit parts A, B and C ask for -- (model, active
    list, parameter-block form: by value for that many datasets, or by pointer) x (storing sweep, and for the fused forms the sweep
    without the store)"""
    seen, out = set(), []
    for c in all_cases():
        key = (c.model, c.K, tuple(c.active), c.kernarg)
        if key not in seen:
            seen.add(key)
            out += [(c.tape(), c.active, c.nd, store) for store in ((True, False) if c.fused else (True,))]
    return out
