"""The integer rules of the GI frame calls (csrc/giframe_rule.h: which call may continue the frame under way, and a history pair's
book-keeping) in a stand-alone host program built with the host sanitizers (tests/giframe_rule_check.cpp).  No GPU is involved."""
import os
import subprocess
import tempfile

import pytest


HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_program(pkg):
    """tests/giframe_rule_check.cpp, compiled for the host alone with AddressSanitizer and UndefinedBehaviorSanitizer"""
    out = os.path.join(tempfile.gettempdir(), "crt_giframe_rule_check_%d" % os.getuid())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc"), os.path.join(HERE, "giframe_rule_check.cpp"), "-o", out])
    return out


def test_continuation_table_and_history_sequences_under_the_host_sanitizers(check_program):
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    # the table alone is 4 kinds under way x 3 asked x 3 counts x 2 settings
    assert int(r.stdout.split()[1]) >= 72 + 20 and not r.stderr.strip(), r.stderr


def test_the_frame_calls_use_the_header_and_keep_no_rule_of_their_own(pkg):
    """crt_giframe.hip asks frame_continues and the ledger; the state it keeps beside them has no flag of the old kind"""
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    text = open(os.path.join(csrc, "crt_giframe.hip")).read()
    for phrase in ('#include "giframe_rule.h"', "frame_continues(", "hist.begin(", "hist.wrote(", "struct History : HistoryLedger"):
        assert phrase in text, phrase
    for gone in ("prog_is_adaptive", "prog_is_split", "has_cur = ", "frames++"):
        assert gone not in text, gone
    # neither file names the other's state, and the queries' file names no frame field
    query = open(os.path.join(csrc, "crt_query.hip")).read()
    assert "crt_query_state" not in text and "crt_giframe_state" not in query
    for field in ("prog_", "den_", "acc_", "->split_", "hist"):
        assert field not in query, field
