"""The slot book (csrc/q3_engine_host.h) for text slots that continue a codec prompt, without a GPU:
tests/engine_host_text_prompt_driver.cpp plays scripts of slot events through SlotBook with `prompt` > 0 and, step by
step, through a stand-in for the counters the device's sampler keeps (n_past from the prompt's length, held on
g = n_past - prompt).  Two things are checked:

  - room, advance, starved, held_next and the held-steps accounting answer exactly what the contract model of
    tests/test_engine_host.py answers for the same script WITHOUT the prompts: the book counts generated frames, a prompt
    changes none of its answers;
  - the book's count of generated frames and of held steps is the device's: generated(b, n_past) == age, held == the steps
    the sampler's rule held the row for.  With the old rule (n_past >= 1 and n_past >= rows) they part at the first step.

CPU only."""
import os
import random
import shutil
import subprocess

import pytest

from tests.test_engine_host import MAX_FRAMES, cells, expect, random_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pdriver(tmp_path_factory):
    assert shutil.which("g++"), "the host rules are tested with g++"
    exe = str(tmp_path_factory.mktemp("engine_host_tp") / "engine_host_text_prompt_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-static-libasan", "-static-libubsan",     # (runs whatever else a process is made to preload)
                           os.path.join(ROOT, "tests", "engine_host_text_prompt_driver.cpp"),
                           "-o", exe])
    return exe


def play(exe, events):
    out = subprocess.run([exe], input="\n".join(events) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(events)
    return lines


def without_prompts(events):
    return [" ".join(e.split()[:4]) if e.startswith("admit") else e for e in events]


def check(exe, events):
    """-> per event ((room, steps), cells) of the driver, after the comparisons of the module docstring."""
    got = [cells(line) for line in play(exe, events)]
    want = [cells(line) for line in expect(without_prompts(events))]
    budget, loose = {}, set()           # per slot: its budget; slots released before their end (their rows stop where they are)
    for i, (ev, (g_head, g_cells), (w_head, w_cells)) in enumerate(zip(events, got, want)):
        where = "event %d (%s) of\n%s" % (i, ev, "\n".join(events[:i + 1]))
        op, *a = ev.split()
        if op == "open":
            budget, loose = {}, set()
        elif op == "admit":
            budget[int(a[0])] = int(a[1])
            loose.discard(int(a[0]))
        elif op == "release":
            loose.add(int(a[0]))
        assert g_head == w_head, where
        for b, (g, w) in enumerate(zip(g_cells, w_cells)):
            assert g[:4] == w, "slot %d at %s\ndriver: %s\nmodel:  %s" % (b, where, g, w)
            if b in budget and b not in loose:
                age, held, _, _, generated, dev_held = g
                assert generated == min(age, budget[b]), "slot %d at %s: %s" % (b, where, g)
                assert dev_held == held, "slot %d at %s: %s" % (b, where, g)
    return got


HAND = {
    # age == 0 with no rows: the prompt's frames are no frame of the slot's own -- the batch stalls, nobody is held
    "age0_no_row_stalls_under_hold": ["open 2 1 16", "admit 0 8 0 0", "admit 1 8 1 9", "run 4", "push 1 1 0", "run 4"],
    "age0_no_row_stalls_without_hold": ["open 2 0 16", "admit 0 8 0 0", "admit 1 8 1 33", "run 4", "push 1 2 0", "run 4", "run 4"],
    # held at g = 1, in the middle, for many steps before the last row; two prompts of different lengths side by side
    "held_beside_moving": ["open 3 1 16", "admit 0 9 0 33", "admit 1 9 1 9", "push 1 2 0", "admit 2 9 1 60", "push 2 1 0",
                           "run 5", "push 2 3 0", "run 2", "run 9"],
    "held_at_g1_middle_and_end": ["open 2 1 24", "admit 0 24 0 0", "admit 1 14 1 33", "push 1 1 0", "run 1", "run 1", "push 1 3 0",
                                  "run 3", "run 2", "push 1 4 0", "run 4", "run 9", "push 1 1 1", "run 9"],
    "every_live_slot_held": ["open 2 1 16", "admit 0 6 1 5", "push 0 1 0", "admit 1 6 1 40", "push 1 2 0", "run 4", "run 4",
                             "release 1", "run 4"],
    "final_push_lifts_the_wait": ["open 1 1 16", "admit 0 7 1 12", "push 0 1 0", "run 3", "run 3", "push 0 0 1", "run 3", "run 9"],
    # budget equal to rows: it ends at its budget, never held, whatever the prompt's length
    "budget_equal_to_rows": ["open 2 1 16", "admit 0 5 1 33", "push 0 5 0", "admit 1 8 0 0", "run 9", "ended 0", "run 9"],
    "budget_equal_to_rows_no_hold": ["open 2 0 16", "admit 0 5 1 33", "push 0 5 0", "admit 1 8 0 0", "run 9", "run 9"],
    # a prompt longer than the budget and than max_frames changes nothing
    "prompt_longer_than_max_frames": ["open 1 1 8", "admit 0 8 1 100", "push 0 3 0", "run 8", "push 0 5 0", "run 8", "run 8"],
    "readmission_forgets_the_prompt": ["open 1 1 16", "admit 0 5 1 20", "push 0 1 0", "run 3", "release 0", "admit 0 4 1 0",
                                       "push 0 2 0", "run 9"],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_rule(pdriver, name):
    check(pdriver, HAND[name])


def test_the_rules_the_scripts_are_named_for(pdriver):
    def runs(name):
        return list(zip(check(pdriver, HAND[name]), HAND[name]))
    r = runs("age0_no_row_stalls_under_hold")
    assert r[3][0][0] == [0, 0] and r[3][0][1][1][:4] == [0, 0, 1, 0]        # starved, not held, no step
    assert r[5][0][0] == [8, 4] and r[5][0][1][1] == [1, 3, 1, 1, 1, 3]      # one frame of its own, then held for 3
    r = runs("age0_no_row_stalls_without_hold")
    assert [x[0][0][1] for x in r if x[1].startswith("run")] == [0, 2, 0]
    r = runs("held_beside_moving")
    assert r[6][0][0] == [9, 5] and [c[:4] for c in r[6][0][1]] == [[5, 0, 0, 0], [2, 3, 1, 1], [1, 4, 1, 1]]
    r = runs("held_at_g1_middle_and_end")
    held = [x[0][1][1][1] for x in r if x[1].startswith("run")]
    assert held == [0, 1, 1, 3, 3, 12, 12]                                   # 1 at g = 1, 2 in the middle, 9 before the last row
    assert r[-1][0][1][1][0] == 14
    r = runs("budget_equal_to_rows")
    assert r[4][0][1][0] == [8, 0, 0, 0, 5, 0]                               # at its budget: never held, the row has ended
    r = runs("prompt_longer_than_max_frames")
    assert [x[0][0][1] for x in r if x[1].startswith("run")] == [3, 5, 0]             # its rows, its budget, nothing
    assert r[3][0][1][0] == [3, 0, 1, 1, 3, 0] and r[5][0][1][0] == [8, 0, 0, 0, 8, 0]


def with_random_prompts(events, seed):
    r = random.Random(5000 + seed)
    return [e + " %d" % r.choice([0, 1, 9, 33, 60]) if e.startswith("admit") else e for e in events]


def test_200_random_scripts_with_prompts(pdriver):
    events = [e for seed in range(200) for e in with_random_prompts(random_script(seed, (1, 2, 5)[seed % 3]), seed)]
    got = check(pdriver, events)
    runs = [g for g, e in zip(got, events) if e.startswith("run")]
    held = sum(sum(c[1] for c in g[1]) for g in runs)
    stalls = sum(g[0] == [0, 0] for g in runs)
    prompted_text = sum(e.startswith("admit") and e.split()[3] == "1" and e.split()[4] != "0" for e in events)
    assert held > 500 and stalls > 100 and prompted_text > 100 and len(events) > 4000 and MAX_FRAMES == 16
