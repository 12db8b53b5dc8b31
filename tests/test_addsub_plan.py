"""The host arithmetic of add_sparse / sub_sparse (csrc/addsub_plan.hpp: the
wave-or-general path rule, the output-at-bound rule, the long rows' chunk
list, the pieces' starts from the chunks' counts and the pinned staging
layout) as a stand-alone CPU program (tests/cpp/addsub_plan_test.cpp), built
with -fsanitize=address,undefined as tests/test_spmm_rule.py builds
spmm_rule.hpp's: longest rows summing to 2047 / 2048 / 2049, either operand
not analysed, BSM_SS_WAVE off / on / unset, the 2^30-byte bound from both
sides at 4- and 8-byte scalars; row sides of 0, 1, LR_CHUNK - 1 .. 2 LR_CHUNK
+ 1 entries with 0, 1 and 3 long rows; M counts 0:4, 3:5, 5:3 and equal,
offsets over 1 to 3 chunks, the two 2^31 limits from both sides; chunk lists
of 0, 1, 255, 256 and 257 bytes."""

from cpp_support import run_sanitized


def test_addsub_plan_under_sanitizer():
    run_sanitized("addsub_plan_test.cpp")
