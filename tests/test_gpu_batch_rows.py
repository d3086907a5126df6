"""Row members in a fused batch (vh_query_agg_batch; PLAN2_PLANE_ROWS): a plan of more than 64 group ids is a candidate like any other, and
a fused launch with such a member runs the row sink for it and the loop over ids for the others (scan_agg_planes_batch_kernel<256, S, rows>).

The table is tests/test_gpu_batch.py's C3Host(3, 5000, 8192) with F = [d2, d3, d4] and ONE V = [d0, d1, d2, m0, count] (10 + 7 + 2 + 10 + 2
planes). GROUP BY d1 has 100 ids, GROUP BY d0 1000; GROUP BY d2 and the totals stay with the loop. Plans run under PLAN_NO_JIT: nothing is
compiled at run time.

ALWAYS, for every member of every batch: tests.parity.compare against the oracle; `agree` bit for bit with dt.query_agg of the same plan and
the same plane_sink; a fused member carries bit 30 on top of exactly its single query's flags and names the batch kernel — ending `, rows>`
exactly when the launch has a row member —, a member that is not fused carries its single query's flags and kernel name."""
import dataclasses

import pytest

from tests.parity import compare
from tests.test_gpu_agg_sliced import agree
from tests.test_gpu_batch import BATCH_KERNEL, BIT30, c3
from tests.test_gpu_batch_share import C3B, member_info
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from tests.test_gpu_plane_agg import C3F, CAP, COUNT, KERNEL, M0, NO_FILTER, NSEG, ROWS, sliced_layouts
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
D0, D1 = 0, 1
AGG, ROWS2 = capi.PLAN2_PLANE_AGG, capi.PLAN2_PLANE_ROWS
RKERNEL = "scan_agg_planes_rows_kernel<"
TAIL = ", rows>"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def host():
    h = C3Host(NSEG, ROWS, CAP)
    h.dt.predpack([D2, D3, D4], sliced=True)                  # F
    h.dt.predpack([D0, D1, D2, M0, COUNT], sliced=True)       # V
    assert len(sliced_layouts(h.dt)) == 2
    yield h
    h.close()


def run(dt, members, launches, label=""):
    """members: test_gpu_batch.Member (fused: what the case expects); launches: per fused launch, whether it has a row member."""
    res, info = dt.query_agg_batch([m.plan for m in members])
    nf = sum(m.fused for m in members)
    print(f"{label}: {info.nplans} plans, {info.fused_groups} fused launch(es) of {info.fused_members} members, {info.singles} single")
    assert (info.nplans, info.fused_groups, info.fused_members, info.singles) == (len(members), len(launches), nf, len(members) - nf), \
        (label, info.fused_groups, info.fused_members, info.singles)
    for r, m in zip(res, members):
        single = dt.query_agg(m.plan)
        print(f"  {m.label}: fused {r.batch_fused}, sink {r.plane_sink} / {single.plane_sink}, flags {r.flags:#x} / {single.flags:#x}, passed {r.passed_recs}, "
              f"groups {r.ngroups}, member {member_info(r)}, kernel {r.kernel} / {single.kernel}")
        compare(r, m.want, m.label + " [batch]")
        compare(single, m.want, m.label + " [single]")
        agree(r, single, m.label)
        assert r.returned == single.returned and r.path == single.path and r.plane_sink == single.plane_sink, (m.label, r.plane_sink, single.plane_sink)
        assert r.batch_fused == m.fused, (m.label, hex(r.flags), r.kernel)
        if m.fused:
            assert r.flags == single.flags | BIT30, (m.label, hex(r.flags), hex(single.flags))
            rows_launch = launches[int(r.batch_member.launch)]
            assert r.kernel.startswith(BATCH_KERNEL) and r.kernel.endswith(TAIL) == rows_launch, (m.label, r.kernel, rows_launch)
            scope = r.kernel[len(BATCH_KERNEL):].split(",")[0].rstrip(">")
            assert single.kernel in (f"{KERNEL}256, {scope}>", f"{RKERNEL}256, {scope}>"), (r.kernel, single.kernel)          # the same memory scope
        else:
            assert r.flags == single.flags and r.kernel == single.kernel and member_info(r) == (0,) * 6, (m.label, hex(r.flags), r.kernel, single.kernel)
    return res, info


def dashboard(h, filt, flags2, row_fused=True):
    """One row member (GROUP BY d1: 100 ids) and two loop members under one filter."""
    return [c3(h, filt, dims=(D1,), flags2=flags2, fused=row_fused, label="GROUP BY d1"),
            c3(h, filt, dims=(D2,), flags2=flags2, label="GROUP BY d2"),
            c3(h, filt, dims=(), flags2=flags2, label="total")]


# ---- (a) one row member and two loop members under one filter: one launch, one mask; the row member leads and follows
def test_a_row_member_joins_the_fused_launch_and_shares_the_mask(host):
    members = dashboard(host, C3F, ROWS2)
    assert 0 < members[0].want.passed_recs < members[0].want.scanned_recs and members[0].want.ngroups > 64
    for order, row_at in ((members, 0), (members[::-1], 2), ([members[1], members[0], members[2]], 1)):
        res, _ = run(host.dt, order, [True], label=f"the row member at position {row_at}")
        assert [r.plane_sink for r in res] == [2 if i == row_at else 1 for i in range(3)]
        assert [member_info(r) for r in res] == [(1, 0, i, 3, 0, 1) for i in range(3)]          # one class; its leader is position 0, whoever that is
        assert len({r.passed_recs for r in res}) == 1
    res, _ = run(host.dt, dashboard(host, NO_FILTER, ROWS2), [True], label="no filter: every row survives")
    assert res[0].passed_recs == NSEG * ROWS and res[0].ngroups == 100


# ---- (b) two row members under different filters
def test_two_row_members_under_different_filters(host):
    members = [c3(host, C3F, dims=(D1,), flags2=ROWS2, label="GROUP BY d1 under C3"), c3(host, C3B, dims=(D0,), flags2=ROWS2, label="GROUP BY d0, one literal moved")]
    assert members[0].want.passed_recs != members[1].want.passed_recs
    res, _ = run(host.dt, members, [True], label="two row members, two filters")
    assert [r.plane_sink for r in res] == [2, 2]
    assert [member_info(r) for r in res] == [(1, 0, 0, 2, 0, 2), (1, 0, 1, 2, 1, 2)]
    res, _ = run(host.dt, members + dashboard(host, C3B, ROWS2)[1:], [True], label="... and two loop members under the second")
    assert [int(r.batch_member.mask_of) for r in res] == [0, 1, 1, 1] and [r.plane_sink for r in res] == [2, 2, 1, 1]


# ---- (c) the same batch with PLAN2_PLANE_AGG only: what it was before this flag
def test_plane_agg_alone_keeps_the_row_member_single(host):
    res, _ = run(host.dt, dashboard(host, C3F, AGG, row_fused=False), [False], label="PLAN2_PLANE_AGG only")
    assert [r.plane_sink for r in res] == [0, 1, 1] and not res[0].plane_agg and RKERNEL not in res[0].kernel
    assert all(not r.kernel.endswith(TAIL) for r in res)
    assert [member_info(r) for r in res[1:]] == [(1, 0, 0, 2, 0, 1), (1, 0, 1, 2, 0, 1)]


# ---- (d) row members whose tables pass 48 KB together: a second launch
def test_tables_beyond_48_kb_open_a_second_launch(host):
    members = [c3(host, C3F, dims=(D0,), flags2=ROWS2, label=f"GROUP BY d0, copy {k}") for k in range(6)]      # 1000 ids, 13 to 17 KB each: at most three fit
    res, info = host.dt.query_agg_batch([m.plan for m in members])
    assert info.fused_groups in (2, 3) and info.fused_members == 6 and info.singles == 0, (info.fused_groups, info.fused_members, info.singles)
    run(host.dt, members, [True] * info.fused_groups, label="six tables of 1000 ids")
    launches = [int(r.batch_member.launch) for r in res]
    assert launches == sorted(launches) and set(launches) == set(range(info.fused_groups)), launches
    assert all(r.plane_sink == 2 and r.kernel.endswith(TAIL) for r in res)


# ---- (e) the hooks that switch sharing and fusion off change no result
def test_no_share_and_no_fuse_give_the_same_results(host, monkeypatch):
    members = dashboard(host, C3F, ROWS2) + [c3(host, C3B, dims=(D0,), flags2=ROWS2, label="GROUP BY d0, one literal moved")]
    base, _ = run(host.dt, members, [True], label="shared")
    assert [int(r.batch_member.mask_classes) for r in base] == [2] * 4
    monkeypatch.setenv("VH_TEST_NO_BATCH_SHARE", "1")
    plain, _ = run(host.dt, members, [True], label="VH_TEST_NO_BATCH_SHARE=1")
    assert [member_info(r) for r in plain] == [(1, 0, i, 4, i, 4) for i in range(4)]
    monkeypatch.delenv("VH_TEST_NO_BATCH_SHARE")
    monkeypatch.setenv("VH_TEST_NO_BATCH_FUSE", "1")
    singles, _ = run(host.dt, [dataclasses.replace(m, fused=False) for m in members], [], label="VH_TEST_NO_BATCH_FUSE=1")
    assert [r.plane_sink for r in singles] == [2, 1, 1, 2] and singles[0].kernel.startswith(RKERNEL)
    for a, b, c, m in zip(base, plain, singles, members):
        agree(a, b, m.label)
        agree(a, c, m.label)
