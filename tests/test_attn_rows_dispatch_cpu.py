"""CPU: csrc/attn_rows.hip follows the arithmetic of the csrc/attention.hip kernels that would run the same shape, so it restates
two facts of that file: the row-tile heuristic (pick_rpw) and the conditions under which the 32-row kernels are launched.  The
restatement is compared with the text of attention.hip here (tests/test_mmaref_cpu.py pins tests/mmaref.py's copy the same way):
if the dispatch there changes, this fails instead of the two paths silently rounding different values."""
import os
import re

import __graft_entry__ as ge


def _src(name):
    return open(os.path.join(ge.CSRC, name)).read()


def _body(text, header):
    i = text.index(header)
    j = text.index("\n}\n", i)
    return re.sub(r"\s+", " ", text[text.index("{", i) + 1:j]).strip()


def test_row_tile_heuristic_is_attention_hips():
    full = _body(_src("attention.hip"), "static inline int pick_rpw(int B, int S, int A)")
    mine = _body(_src("attn_rows.hip"), "static inline int full_rows_per_workgroup(int B, int S, int A)")
    assert mine == full


def test_launch_conditions_restated():
    att, rows = _src("attention.hip"), _src("attn_rows.hip")
    # forward: the 32-row kernel without dropout, for S a multiple of 64 from 192 on, when the row tile is whole 32-row passes;
    # two key parts wherever attn_rows.hip's waves can follow them (S % 128 == 0 <=> NKB % 8 == 0 there)
    assert "constexpr bool CAN_ROWS32 = !DROP && NKB % 4 == 0 && NKB >= 12;" in att
    assert "if (rows32 && rpw % 256 == 0) {" in att
    assert "#define KBNER_ATTN_PARTS 2" in att and "constexpr int NP = (NKB % 8 == 0) ? KBNER_ATTN_PARTS : 2;" in att
    assert "const bool rows32 = true;" in att
    assert "(S >= 192 && S % 128 == 0 && full_rows_per_workgroup(B, S, A) % 256 == 0) ? 1 : 0;" in rows
    # backward: the 32-row kernels whenever the row tile is whole 32-row passes (S % 32 == 0 always holds: S % 64 == 0 is checked)
    assert "if (rpw % 256 == 0 && S % 32 == 0) {" in att
    assert "const int fused = full_rows_per_workgroup(B, S, A) % 256 == 0 ? 1 : 0;" in rows
