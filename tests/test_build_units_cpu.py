"""build.UNITS against the real include graph of csrc/.  The library is built unit by unit, and a unit is recompiled when one of the headers
build.py lists for it is newer than its object: a header the list lacks means a silently stale library, and a header the main unit does not
need means a 2-minute rebuild where 5 seconds would do.  Reads source text only.  No GPU, no compiler."""
import importlib
import os
import re

build = importlib.import_module("batch-scheduler_amd.build")
CSRC = build.CSRC
FAMILY_HEADERS = {"bs_preempt.hpp", "bs_preempt_commit.hpp", "bs_preempt_commit_gang.hpp", "bs_bound_apply.hpp", "bs_pdb.hpp", "bs_seq.hpp",
                  "bs_seq_expire.hpp", "bs_seq_expire_list.hpp"}
MAIN_HEADERS = {"bs_fast.hpp", "bs_filter_t.hpp", "bs_epoch.hpp", "bs_queue.hpp"}


def closure(unit):
    """every header the unit reaches through quoted #includes, as paths relative to csrc/ (the .hip includes exist under BS_UNITY only)"""
    seen, todo = set(), [unit]
    while todo:
        here = todo.pop()
        text = open(os.path.join(CSRC, here)).read()
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, re.M):
            if inc.endswith(".hip"):
                continue
            rel = os.path.normpath(os.path.join(os.path.dirname(here), inc))
            assert os.path.exists(os.path.join(CSRC, rel)), (here, inc)
            if rel not in seen:
                seen.add(rel)
                todo.append(rel)
    return seen


CLOSURE = {unit: closure(unit) for unit in build.UNITS}


def test_every_header_a_unit_reaches_is_listed_for_it():
    assert list(build.UNITS) == build.SOURCES == ["bsched.hip", "tu_fast.hip", "tu_seq.hip", "tu_seq_expire.hip", "tu_preempt.hip"]
    for unit, listed in build.UNITS.items():
        missing = CLOSURE[unit] - {os.path.normpath(h) for h in listed}
        assert not missing, (unit, sorted(missing))


def test_the_main_unit_depends_on_no_family_header():
    assert not FAMILY_HEADERS & set(build.UNITS["bsched.hip"])
    assert not FAMILY_HEADERS & CLOSURE["bsched.hip"]


def test_the_family_units_depend_on_no_header_of_the_batch_chains():
    for unit in ("tu_preempt.hip", "tu_seq.hip", "tu_seq_expire.hip"):
        assert not MAIN_HEADERS & CLOSURE[unit], unit


def test_no_header_fences_itself_against_the_main_unit():
    """BS_TU_MAIN appears in a conditional only where bs_common.hpp turns it into the emit switches"""
    for name in sorted(os.listdir(CSRC)):
        lines = [l for l in open(os.path.join(CSRC, name)).read().splitlines() if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", l) and "BS_TU_MAIN" in l]
        assert len(lines) == (1 if name == "bs_common.hpp" else 0), (name, lines)
