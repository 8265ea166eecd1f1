"""The ways of reaching a tracking kernel (`k_track_*` in csrc/), one row per way: entry point, selector, patch
sizes, the environment of the context, and the template arguments of every kernel the launch runs -- for LEAN
parameters (no regularisation penalty, solver_variant 0) and for generic ones (everything else).

Plain data: nothing here imports the package or touches a device.  test_track_routes_cpu.py holds the table against the
kernel names of the build (every symbol claimed, every claim built); test_instantiations_gpu.py runs the rows.

A kernel is written as (template name, template arguments), booleans as 0 / 1:
    ("k_track_block", (2, 25, 4, 0, 0, 1))  is  k_track_block<2, 25, 4, false, false, true>
Template parameters (csrc/pagk_kernels.h, pagk_wave_kernel.h, pagk_quad_kernel.h, pagk_rows_kernel.h):
    k_track_block<NR, TAIL, WAVES, MFMA, RELAXED, LEAN>     k_track_wave<NCH, TAIL, LEAN>
    k_track_block5 / k_track_resume / k_track_resume_live / k_track_block_pyr<NR, TAIL, LEAN>
    k_track_quad<NCH, LEAN, LEVELS, BATCH>                  k_track_rows<NCH>           k_track_thread
with P = (2h + 1)^2 pixels per patch: NR = ceil(P / (64 * WAVES)), TAIL = P mod 32, NCH = ceil(P / 64)."""
import dataclasses
import re

# (NR, TAIL) of the 4-wave kernels for every half patch the library accepts (the kernel table of csrc/pagk_hip.hip
# builds them from patch_shape in csrc/pagk_select.h; this is the independent restatement it is checked against)
BLOCK_ARGS = {1: (1, 9), 2: (1, 25), 3: (1, 17), 4: (1, 17), 5: (1, 25), 6: (1, 9), 7: (1, 1), 8: (2, 1), 9: (2, 9),
              10: (2, 25), 11: (3, 17), 12: (3, 17), 13: (3, 25), 14: (4, 9), 15: (4, 1)}
# the patch sizes of the throughput kernels, the continuation and the fused launch: NCH, and (NR, TAIL) of the 2-wave form
NCH = {5: 2, 7: 4, 10: 7}
MFMA_ARGS = {5: (1, 25), 7: (2, 1), 10: (4, 25)}
COMMON = (5, 7, 10)


def _thread(h, lean):
    return [("k_track_thread", ())]


def _block(h, lean):
    return [("k_track_block", BLOCK_ARGS[h] + (4, 0, 0, int(lean)))]


def _block5(h, lean):   # generic parameters fall back to the pipelined 4-wave kernel
    return [("k_track_block5", BLOCK_ARGS[h] + (1,))] if lean else _block(h, lean)


def _mfma(h, lean):
    return [("k_track_block", MFMA_ARGS[h] + (2, 1, 0, int(lean)))]


def _wave(h, lean):
    return [("k_track_wave", (NCH[h], BLOCK_ARGS[h][1], int(lean)))]


def _quad(h, lean):
    return [("k_track_quad", (NCH[h], int(lean), 0, 0))]


def _levels(h, lean):
    return [("k_track_quad", (NCH[h], int(lean), 1, 0))]


def _batch(h, lean):
    return [("k_track_quad", (NCH[h], int(lean), 1, 1))]


def _rows(h, lean):   # one instantiation serves both
    return [("k_track_rows", (NCH[h],))]


def _sweep(h, lean):
    return [("k_track_resume", BLOCK_ARGS[h] + (int(lean),))]


def _finisher(h, lean):
    return [("k_track_resume_live", BLOCK_ARGS[h] + (int(lean),))]


def _fused(h, lean):
    return [("k_track_block_pyr", BLOCK_ARGS[h] + (int(lean),))]


def _relaxed(h, lean):   # one instantiation serves both
    return [("k_track_block", BLOCK_ARGS[h] + (4, 0, 1, 0))]


@dataclasses.dataclass(frozen=True)
class Route:
    name: str
    entry: str                 # Context method that launches: "track", "track_device_fused", "track_device_batch"
    selectors: tuple           # pagk_set_kernel values the row runs (the lead context's, for the batch)
    halves: tuple              # half patch sizes
    env: tuple                 # ((name, value), ...): environment of the row's own context; () = the shared context
    variants: tuple            # pagk_last_variant per selector
    handover: bool             # pagk_last_handover > 0 after the launch
    kernels: tuple             # per selector, the functions (h, lean) -> kernels that the launch runs
    needs_variant: int = 0     # the row needs a library built with -DPAGK_ALL_VARIANTS (variants 2 and 6)
    test: str = "test_instantiations_gpu.py::test_route"   # the test that runs the row

    def claims(self, h, lean):
        return [k for per_selector in self.kernels for f in per_selector for k in f(h, lean)]


_CONT = (("PAGK_QUAD_BUDGET", "3"), ("PAGK_SUSPEND_LONE", "0"))

ROUTES = (
    Route("thread", "track", (1,), (5, 10, 15), (), (1,), False, ((_thread,),)),
    Route("block", "track", (0,), tuple(range(1, 16)), (), (0,), False, ((_block,),)),
    Route("block5", "track", (0,), (10,), (("PAGK_BLOCK5_MIN", "1"),), (0,), False, ((_block5,),)),
    Route("wave", "track", (3,), COMMON, (), (3,), False, ((_wave,),)),
    Route("quad", "track", (5,), COMMON, (("PAGK_QUAD_BUDGET", "0"),), (5,), False, ((_quad,),)),
    Route("levels", "track", (7,), COMMON, (("PAGK_QUAD_BUDGET", "0"),), (7,), False, ((_levels,),)),
    # hand-over after 3 iterations, every feature (not only a wave's last): live finisher beside the throughput kernel
    # plus the sweep behind it; the sweep alone; a finisher that gives up at its first look
    Route("continuation-live", "track", (5, 7), COMMON, _CONT, (5, 7), True,
          ((_quad, _finisher, _sweep), (_levels, _finisher, _sweep))),
    Route("continuation-sweep", "track", (5, 7), COMMON, _CONT + (("PAGK_FINISHER_WGS", "0"),), (5, 7), True,
          ((_quad, _sweep), (_levels, _sweep))),
    Route("continuation-impatient", "track", (5, 7), COMMON, _CONT + (("PAGK_FINISHER_POLLS", "0"),), (5, 7), True,
          ((_quad, _finisher, _sweep), (_levels, _finisher, _sweep))),
    # the next frame's pyramid (even parents, <= 4 levels) built by trailing workgroups of the 4-wave launch
    Route("fused", "track_device_fused", (0,), COMMON, (), (0,), False, ((_fused,),)),
    # three streams of 1, 67 and 30 features on two frame sizes as one launch of the lead context
    Route("batch", "track_device_batch", (7,), COMMON, (), (7,), False, ((_batch,),)),
    Route("relaxed", "track", (4,), (10,), (), (4,), False, ((_relaxed,),),
          test="test_parity_gpu.py::test_relaxed_order_experiment"),
    Route("mfma", "track", (2,), COMMON, (), (2,), False, ((_mfma,),), needs_variant=2),
    Route("rows", "track", (6,), COMMON, (), (6,), False, ((_rows,),), needs_variant=6),
)

# Built kernels that no row runs, each with its reason.
EXEMPT = {
    ("k_track_block", (1, 25, 4, 0, 1, 0)): "relaxed-order experiment at h = 5: not parity-exact, never selected "
                                            "automatically; h = 10 stands for it in test_relaxed_order_experiment",
    ("k_track_block", (1, 1, 4, 0, 1, 0)): "relaxed-order experiment at h = 7: not parity-exact, never selected "
                                           "automatically; h = 10 stands for it in test_relaxed_order_experiment",
}


def route(name):
    return next(r for r in ROUTES if r.name == name)


def claimed():
    """{kernel: [(route name, h, 'lean' | 'generic'), ...]} over every row of the product build (the needs_variant rows'
    kernels are not in it)."""
    out = {}
    for r in ROUTES:
        if r.needs_variant:
            continue
        for h in r.halves:
            for lean in (True, False):
                for k in r.claims(h, lean):
                    out.setdefault(k, []).append((r.name, h, "lean" if lean else "generic"))
    return out


_ARG = re.compile(r"L([ib])(\d+)E")


def parse_symbol(symbol):
    """Itanium-mangled kernel name -> (template name, template arguments), or None when it is no tracking kernel:
    '_ZN4pagk13k_track_blockILi2ELi25ELi4ELb0ELb0ELb1EEEvNS_9TrackArgsE' -> ('k_track_block', (2, 25, 4, 0, 0, 1))."""
    m = re.match(r"_ZN4pagk\d+(k_track_[a-z0-9_]+?)(?:I((?:L[ib]\d+E)+)E)?(?:Ev|E)N", symbol)
    if not m:
        return None
    return m.group(1), tuple(int(v) for _, v in _ARG.findall(m.group(2) or ""))
