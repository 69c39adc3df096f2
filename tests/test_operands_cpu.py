"""Which codebook-derived operands are current (csrc/codebook_operands.hpp, operands::State) without a GPU, through the library's
test hook som_operands_replay (include/somhip_test.h).

The oracle is a small model of the BUFFERS: the codebook has a version number, every operand carries the version it was built from
(the float32 image also its order), and every kernel the host code launches for a listed rebuild reads and writes what its launch
site in somhip.hip passes it.  Every event sequence of length 4 over a configuration's alphabet is replayed (the checks run per
event, so the shorter sequences are their prefixes) and two things are asserted:
  SOUNDNESS  after a request, every operand its reader reads is at the codebook's version and in the requested order, and every
             rebuild read current inputs; a deferred 16-bit image is owed until it is taken, and only the deferring launch may go on
  ECONOMY    no listed rebuild targets an operand that was already current in the right order."""
import ctypes as C
import itertools

import pytest

from xpysom_dask_amd import _lib

# events and requests of som_operands_replay
REPLACED, MERGE_PLAIN, MERGE_HALF, MERGE_EXACT, REQUEST, TAKE, REPLAY, CANARY = range(8)
SEARCH, F32_UNITS, EXACT_SCREEN = range(3)
WSQ, PERMUTE, F32, F32_PATCH, HALF, SKIP_NORMS, DEFERRED, CM, FLUSH, FLUSH_CM, A_PATCH, A_PENDING, A_CEN, A_INSTEP = range(14)


def cfg(half=0, exact=0, patch=0, cosine=0, resident=0, f32_stage=1):
    return (half, exact, patch, cosine, resident, f32_stage)


# (config, do the handle's fused merges write the plan's centroids)
CONFIGS = {
    "f32": (cfg(), 0),
    "bf16-euclidean": (cfg(half=1), 0),
    "bf16-cosine": (cfg(half=1, cosine=1), 0),
    "exact-resident": (cfg(half=1, exact=1, resident=1), 0),
    "exact-resident-cen": (cfg(half=1, exact=1, resident=1), 1),
    "exact-resident-patch": (cfg(half=1, exact=1, patch=1, resident=1), 0),
    "exact-resident-patch-cen": (cfg(half=1, exact=1, patch=1, resident=1), 1),
    "exact-wide-euclidean": (cfg(half=1, exact=1, patch=1, f32_stage=0), 0),
    "exact-wide-cosine": (cfg(half=1, exact=1, patch=1, cosine=1, f32_stage=0), 0),
}


def replay(config, script):
    lib = _lib.load()
    n = len(script)
    flat = [x for e in script for x in e]
    out = (C.c_int32 * (14 * n))()
    assert lib.som_operands_replay((C.c_int32 * 6)(*config), n, (C.c_int32 * (3 * n))(*flat), out) == 0
    return [list(out[14 * i:14 * i + 14]) for i in range(n)]


def alphabet(config, cen):
    half, exact, patch, cosine, resident, f32_stage = config
    ev = [(REPLACED, 0, 0), (MERGE_PLAIN, 0, 0), (REQUEST, SEARCH, 0), (REQUEST, F32_UNITS, 0), (TAKE, 0, 0), (CANARY, 0, 0)]
    if half and not exact:
        ev.append((MERGE_HALF, 0, 0))
    if exact:
        ev.append((REQUEST, EXACT_SCREEN, 0))
    if resident:
        ev += [(MERGE_EXACT, 0, cen), (REQUEST, SEARCH, 1)]
    if not exact:
        ev.append((REPLAY, SEARCH, 0))
    return ev


class Buffers:
    """The model: version 0 = never built."""

    def __init__(self, config):
        self.half_, self.exact, self.patch, self.cosine, self.resident, self.f32_stage = config
        self.config = config
        self.v = 1
        self.wsq = self.wsqp = self.wp = self.half = self.norms = self.cen = 0
        self.f32 = (0, 0)            # (version, in patch order)
        self.owed = False            # the 16-bit image's kernel is left to a launch
        self.in_step = 0             # the state's last answer to "is the patch-order copy in step"

    def changed(self):
        self.v += 1
        self.owed = False

    def image_kernel(self, cm):      # prep_w_exact_k16_kernel, alone or inside exact_prep_images_kernel
        assert not self.patch or self.wp == self.v
        assert not cm or self.cen == self.v
        self.half, self.owed = self.v, False

    def rebuild(self, o, economy=True):
        v = self.v
        if o[FLUSH]:
            assert self.owed
            self.image_kernel(o[FLUSH_CM])
        if o[WSQ]:                   # row_sq_f32_kernel(W -> wsq, wsq_p)
            assert not economy or self.wsq != v or (self.patch and self.wsqp != v)
            self.wsq = v
            self.wsqp = v if self.patch else 0
        if o[PERMUTE]:               # exact_permute_kernel(W, wsq -> Wp, wsq_p)
            assert self.patch and self.wsq == v
            assert not economy or self.wp != v or self.wsqp != v
            self.wp = self.wsqp = v
        if o[F32]:                   # prep_tiles_f32_kernel / prep_w_f32_res_kernel from (Wp, wsq_p) or (W, wsq)
            assert not economy or self.f32 != (v, o[F32_PATCH])
            assert (self.wp == v and self.wsqp == v) if o[F32_PATCH] else self.wsq == v
            self.f32 = (v, o[F32_PATCH])
        if o[HALF]:                  # prep_codebook_half
            assert self.half_ and (not economy or self.half != v)
            if self.exact:
                assert not self.patch or self.wp == v
                if o[SKIP_NORMS]:
                    assert self.resident and self.norms == v
                else:
                    assert (self.wsqp if self.patch else self.wsq) == v
                self.norms = 0       # (the image kernel leaves its error maximum in the pair)
                if o[DEFERRED]:
                    assert self.resident
                    self.owed = True
                    assert not o[CM] or self.cen == v
                elif self.resident:
                    self.image_kernel(o[CM])
                else:
                    self.half = v
            else:
                assert not self.cosine or self.wsq == v
                self.half = v

    def reader(self, rq, may_defer, o):
        v = self.v
        patch = self.patch and (rq == EXACT_SCREEN or (rq == SEARCH and self.exact))
        if rq != SEARCH or not self.half_ or self.exact:
            assert self.wsq == v and self.f32 == (v, patch)
            assert not patch or (self.wp == v and self.wsqp == v)
        if self.half_ and rq != F32_UNITS:
            assert self.half == v or (may_defer and self.owed and o[A_PENDING])
            assert may_defer or not self.owed

    def apply(self, ev, o):
        kind, rq, flag = ev
        if kind == REPLACED:
            self.changed()
        elif kind == MERGE_PLAIN:    # merge_kernel writes Wp beside W where the state said it was in step
            in_step = self.in_step
            assert not in_step or self.wp == self.v
            self.changed()
            if in_step:
                self.wp = self.v
        elif kind == MERGE_HALF:     # merge_prep_half: the 16-bit image and its norms
            self.changed()
            self.half = self.v
        elif kind == MERGE_EXACT:    # exact_merge_prep_kernel
            self.changed()
            v = self.v
            self.wsq = self.norms = v
            if self.patch:
                self.wp = self.wsqp = v
            if self.f32_stage:
                self.f32 = (v, self.patch)
            if flag:
                self.cen = v
        elif kind == REQUEST:
            self.rebuild(o)
            self.reader(rq, flag, o)
        elif kind == TAKE:
            assert o[FLUSH] == self.owed
            if o[FLUSH]:
                self.image_kernel(o[FLUSH_CM])
        elif kind == REPLAY:         # the captured epoch: a refresh from the all-stale state, whatever is current
            self.rebuild(replay(self.config, [(REQUEST, rq, 0)])[0], economy=False)
            self.reader(rq, 0, o)
        elif kind == CANARY:         # verify_best_kernel reads W and |w|^2
            self.rebuild(o)
            assert self.wsq == self.v
        if kind not in (REQUEST, CANARY):
            assert not any(o[:8])
        # the accessors never claim more than the buffers hold
        assert o[A_PENDING] == self.owed
        assert o[A_PATCH] == self.f32[1]
        assert not o[A_CEN] or self.cen == self.v
        assert not o[A_INSTEP] or self.wp == self.v
        self.in_step = o[A_INSTEP]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_sequence_is_sound_and_economical(name):
    config, cen = CONFIGS[name]
    for script in itertools.product(alphabet(config, cen), repeat=4):
        outs = replay(config, script)
        m = Buffers(config)
        for i, (ev, o) in enumerate(zip(script, outs)):
            try:
                m.apply(ev, o)
            except AssertionError as e:
                raise AssertionError("%s: event %d of %r -> %r" % (name, i, script, o)) from e


@pytest.mark.parametrize("name", ["exact-resident-cen", "exact-resident-patch", "exact-resident-patch-cen"])
def test_search_after_exact_fused_merge_lists_only_the_half_image(name):
    config, cen = CONFIGS[name]
    for defer in (0, 1):
        o = replay(config, [(MERGE_EXACT, 0, cen), (REQUEST, SEARCH, defer)])[1]
        assert o[:10] == [0, 0, 0, 0, 1, 1, defer, cen, 0, 0]
        assert o[A_PENDING] == defer and o[A_CEN] == cen and o[A_PATCH] == config[2]


def test_switching_the_float32_order_rebuilds_the_float32_image_alone():
    config, _ = CONFIGS["exact-resident-patch"]
    outs = replay(config, [(REPLACED, 0, 0), (REQUEST, EXACT_SCREEN, 0), (REQUEST, F32_UNITS, 0), (REQUEST, EXACT_SCREEN, 0),
                           (REQUEST, EXACT_SCREEN, 0)])
    assert outs[1][:10] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert outs[2][:10] == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0] and outs[2][A_PATCH] == 0
    assert outs[3][:10] == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0] and outs[3][A_PATCH] == 1
    assert outs[4][:10] == [0] * 10


@pytest.mark.parametrize("name", ["f32", "bf16-euclidean", "bf16-cosine"])
def test_graph_replayed_equals_a_refresh_from_all_stale(name):
    config, _ = CONFIGS[name]
    for merge in (MERGE_PLAIN,) + ((MERGE_HALF,) if config[0] else ()):
        for rq in (SEARCH, F32_UNITS):
            head = [(REQUEST, F32_UNITS, 0), (merge, 0, 0)]
            a = replay(config, head + [(REPLAY, SEARCH, 0), (REQUEST, SEARCH, 0), (merge, 0, 0), (REPLAY, SEARCH, 0), (REQUEST, rq, 0)])
            b = replay(config, head + [(REPLACED, 0, 0), (REQUEST, SEARCH, 0), (REQUEST, SEARCH, 0), (merge, 0, 0), (REPLACED, 0, 0),
                                       (REQUEST, SEARCH, 0), (REQUEST, rq, 0)])
            assert a[3][:10] == [0] * 10 == b[4][:10]          # (the search's operands are current behind a replay)
            assert a[-1] == b[-1]


def test_bad_arguments_are_refused():
    lib = _lib.load()
    ok = (C.c_int32 * 6)(*cfg(half=1))
    one = (C.c_int32 * 3)(REQUEST, SEARCH, 0)
    out = (C.c_int32 * 14)()
    assert lib.som_operands_replay(ok, 1, one, out) == 0
    assert lib.som_operands_replay(None, 1, one, out) != 0
    assert lib.som_operands_replay(ok, -1, one, out) != 0
    assert lib.som_operands_replay((C.c_int32 * 6)(*cfg(exact=1)), 1, one, out) != 0          # exact without a 16-bit image
    assert lib.som_operands_replay(ok, 1, (C.c_int32 * 3)(9, 0, 0), out) != 0
    assert lib.som_operands_replay(ok, 1, (C.c_int32 * 3)(REQUEST, 3, 0), out) != 0
    assert lib.som_operands_replay(ok, 1, (C.c_int32 * 3)(MERGE_EXACT, 0, 0), out) != 0     # no resident exact path
