"""The engine's host rules (csrc/q3_engine_host.h: the slot book behind q3e_run / q3e_text_state / q3e_text_held, and the
prefix cache's index behind q3e_admit_keyed) without a GPU: tests/engine_host_driver.cpp is built with g++, fed scripts of
events and compared line by line with a model written here from the contract text of include/qwen3tts_engine.h (q3e_run,
q3e_text_hold, q3e_text_state, q3e_prefix_cache).  The same rules are what the scheduler tests' stand-in engines
(TextFakeEngine, HoldFakeEngine) play, so scripts are replayed through those as well.  CPU only."""
import dataclasses
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_concurrent_scheduler import DEFAULTS
from tests.test_text_hold_scheduler import HoldFakeEngine
from tests.test_text_stream_scheduler import TextFakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_FRAMES = 16     # the engine's max_frames in the scripts (budgets are <= 12)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert shutil.which("g++"), "the host rules are tested with g++"
    exe = str(tmp_path_factory.mktemp("engine_host") / "engine_host_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-static-libasan", "-static-libubsan",     # (runs whatever else a process is made to preload)
                           os.path.join(ROOT, "tests", "engine_host_driver.cpp"), "-o", exe])
    return exe


def play(driver, events):
    out = subprocess.run([driver], input="\n".join(events) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(events)
    return lines


# ---------------------------------------------------------------------------------------------------------------------
# the model: include/qwen3tts_engine.h, per-slot mode and "Text streamed into a running utterance"


class Model:
    def __init__(self, B, hold, max_frames=MAX_FRAMES):
        self.B, self.hold, self.cap = B, bool(hold), max_frames
        self.s = [None] * B      # per slot that ever held an utterance: its record

    def admit(self, b, budget, text):
        self.s[b] = dict(budget=budget, frames=0, held=0, live=True, text=bool(text), rows=0, final=False)

    def push(self, b, n, final):
        self.s[b]["rows"] += n
        self.s[b]["final"] |= bool(final)

    def end(self, b):                # q3e_release, or q3e_get_done reporting the slot
        if self.s[b]:
            self.s[b]["live"] = False

    def live(self):
        return [s for s in self.s if s and s["live"]]

    @staticmethod
    def text_open(s):                # "a live text slot" whose text has not ended and that still has a frame to emit
        return s["live"] and s["text"] and not s["final"] and s["frames"] < s["budget"]

    def starved(self, s):            # "... WITHOUT a row for its next frame"
        return bool(s) and self.text_open(s) and s["rows"] <= s["frames"]

    def held(self, s):               # hold mode: starved, with a step of its own to repeat
        return self.hold and self.starved(s) and s["frames"] >= 1

    def _step(self):
        """One frame step: held slots are held, every other slot that was ever admitted counts it (an ended row steps on,
        its counter stops at the end of the codes array)."""
        for s in self.s:
            if not s:
                continue
            if self.held(s):
                s["held"] += 1
            else:
                s["frames"] = min(s["frames"] + 1, self.cap)

    def run(self, n):
        if not self.hold:
            # never past the largest budget a live slot has left, never past the rows a live text slot has
            room = max([s["budget"] - s["frames"] for s in self.live()], default=0)
            room = min([room] + [s["rows"] - s["frames"] for s in self.live() if self.text_open(s)])
            steps = max(0, min(n, room))
            for _ in range(steps):
                self._step()
            return steps
        # hold: a text slot with no frame yet and no row stalls the batch; else step while some live slot still emits
        if any(self.text_open(s) and s["frames"] == 0 and s["rows"] == 0 for s in self.live()):
            return 0
        steps = 0
        while steps < n and any(not self.held(s) and s["frames"] < s["budget"] for s in self.live()):
            self._step()
            steps += 1
        return steps

    def room(self):
        return copy_of(self).run(10 ** 6)

    def line(self, room, steps):
        cells = ["-1 0 0 0" if not s else "%d %d %d %d" % (s["frames"], s["held"], self.starved(s), self.held(s)) for s in self.s]
        return " | ".join(["slots %d %d" % (room, steps)] + cells)


def copy_of(m):
    c = Model(m.B, m.hold, m.cap)
    c.s = [dict(s) if s else None for s in m.s]
    return c


def expect(events):
    """The lines the contract asks for, for a script of slot events."""
    m, out = None, []
    for ev in events:
        op, *a = ev.split()
        a = [int(x) for x in a]
        steps, room = 0, None
        if op == "open":
            m = Model(a[0], a[1], a[2] if len(a) > 2 else 64)
        elif op == "admit":
            m.admit(*a)
        elif op == "push":
            m.push(*a)
        elif op in ("ended", "release"):
            m.end(a[0])
        elif op == "run":
            room = m.room()
            steps = m.run(a[0])
        out.append(m.line(m.room() if room is None else room, steps))
    return out


def check(driver, events):
    got, want = play(driver, events), expect(events)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "event %d (%s) of\n%s\ndriver: %s\nmodel:  %s" % (i, events[i], "\n".join(events[:i + 1]), g, w)
    return got


def cells(line):
    head, *rest = line.split(" | ")
    return [int(x) for x in head.split()[1:]], [[int(x) for x in c.split()] for c in rest]


# ---------------------------------------------------------------------------------------------------------------------
# one hand-written script per rule

HAND = {
    "largest_budget_left": ["open 2 0 16", "admit 0 3 0", "admit 1 5 0", "run 4", "run 4", "ended 0", "ended 1", "run 4"],
    "stall_without_hold": ["open 2 0 16", "admit 0 8 0", "admit 1 8 1", "run 4", "push 1 2 0", "run 4", "run 4", "push 1 1 0", "run 4"],
    "age0_no_row_stalls_under_hold": ["open 2 1 16", "admit 0 8 0", "admit 1 8 1", "run 4", "push 1 1 0", "run 4"],
    "held_beside_moving": ["open 3 1 16", "admit 0 9 0", "admit 1 9 1", "push 1 2 0", "admit 2 9 1", "push 2 1 0", "run 5",
                           "push 2 3 0", "run 2", "run 9"],
    "every_live_slot_held": ["open 2 1 16", "admit 0 6 1", "push 0 1 0", "admit 1 6 1", "push 1 2 0", "run 4", "run 4",
                             "release 1", "run 4"],
    "final_push_lifts_the_wait": ["open 1 1 16", "admit 0 7 1", "push 0 1 0", "run 3", "run 3", "push 0 0 1", "run 3", "run 9"],
    "final_push_without_hold": ["open 1 0 16", "admit 0 7 1", "push 0 2 0", "run 5", "push 0 0 1", "run 9"],
    "budget_reached_while_waiting": ["open 2 1 16", "admit 0 2 1", "push 0 5 0", "admit 1 6 0", "run 9", "run 1", "ended 0",
                                     "ended 1", "run 1"],
    "budget_reached_while_waiting_no_hold": ["open 2 0 16", "admit 0 2 1", "push 0 2 0", "admit 1 6 0", "run 9", "run 9"],
    "max_frames_caps_the_counters": ["open 2 0 8", "admit 0 2 0", "run 2", "ended 0", "admit 1 8 0", "run 8", "ended 1",
                                     "admit 1 8 0", "run 8"],
    "max_frames_caps_under_hold": ["open 2 1 8", "admit 0 3 1", "push 0 1 0", "release 0", "admit 1 8 0", "run 8", "ended 1",
                                   "admit 1 8 0", "run 8"],
    "readmission_restarts_the_slot": ["open 1 1 16", "admit 0 5 1", "push 0 1 0", "run 3", "release 0", "admit 0 4 0", "run 9"],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_rule(driver, name):
    check(driver, HAND[name])


def test_the_rules_the_scripts_are_named_for(driver):
    """What each hand-written script is about did happen in it (the model and the driver could agree on something else)."""
    def runs(name):
        ev = HAND[name]
        return [(cells(line), e) for line, e in zip(play(driver, ev), ev)]
    r = runs("age0_no_row_stalls_under_hold")
    assert r[3][0][0] == [0, 0] and r[5][0][0][1] == 4                      # no step, then the steps
    r = runs("held_beside_moving")
    assert r[6][0][0] == [9, 5] and r[6][0][1] == [[5, 0, 0, 0], [2, 3, 1, 1], [1, 4, 1, 1]]
    r = runs("every_live_slot_held")
    assert r[5][0][0] == [2, 2] and r[6][0][0] == [0, 0] and r[8][0][0] == [0, 0]
    r = runs("final_push_lifts_the_wait")
    assert [x[0][0][1] for x in r if x[1].startswith("run")] == [1, 0, 3, 3]
    r = runs("budget_reached_while_waiting")
    assert r[4][0][0] == [6, 6] and r[4][0][1][0] == [6, 0, 0, 0]          # at its budget: neither starved nor held, it steps on
    r = runs("max_frames_caps_the_counters")
    assert r[-1][0][1] == [[8, 0, 0, 0], [8, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# seeded random scripts


def random_script(seed, B):
    r = random.Random(seed)
    hold = r.randrange(2)
    ev = ["open %d %d %d" % (B, hold, MAX_FRAMES)]
    m = Model(B, hold)
    for _ in range(40):
        free = [b for b in range(B) if not (m.s[b] and m.s[b]["live"])]
        texts = [b for b in range(B) if m.s[b] and m.s[b]["live"] and m.s[b]["text"] and not m.s[b]["final"]]
        over = [b for b in range(B) if m.s[b] and m.s[b]["live"] and m.s[b]["frames"] >= m.s[b]["budget"]]
        live = [b for b in range(B) if m.s[b] and m.s[b]["live"]]
        op = r.choice(["admit", "admit", "push", "push", "push", "run", "run", "run", "ended", "ended", "release"])
        if op == "admit" and free:
            a = (r.choice(free), r.randint(1, 12), r.randrange(2))
            m.admit(*a)
            if a[2] and r.random() < 0.7:      # a server admits a text slot with its first rows at hand
                ev.append("admit %d %d %d" % a)
                a = (a[0], r.randint(1, 3), 0)
                op = "push"
                m.push(*a)
        elif op == "push" and texts:
            b = r.choice(texts)
            a = (b, min(r.randrange(4), MAX_FRAMES - m.s[b]["rows"]), int(r.random() < 0.25))
            m.push(*a)
        elif op == "run":
            a = (r.randint(1, 5),)
            m.run(*a)
        elif op == "ended" and over:
            a = (r.choice(over),)
            m.end(*a)
        elif op == "release" and live:
            a = (r.choice(live),)
            m.end(*a)
        else:
            continue
        ev.append(" ".join([op] + [str(x) for x in a]))
    return ev


RANDOM = [(seed, (1, 2, 5)[seed % 3]) for seed in range(200)]


def test_200_random_scripts(driver):
    events = [e for seed, B in RANDOM for e in random_script(seed, B)]     # (every `open` begins a new batch)
    got = check(driver, events)
    held = sum(sum(c[1] for c in cells(g)[1]) for g, e in zip(got, events) if e.startswith("run"))
    stalls = sum(cells(g)[0] == [0, 0] for g, e in zip(got, events) if e.startswith("run"))
    assert held > 500 and stalls > 100 and len(events) > 4000              # the scripts do reach the rules


# ---------------------------------------------------------------------------------------------------------------------
# the scheduler tests' stand-in engines play the same rules


def replay_through_fake(driver, seed, B, hold):
    """A random session of the fake engine, mirrored event by event into a driver script; -> per event the fake's (steps,
    frames, held, starved) and whether the slot is one the fake still steps.  One step per run: the fake ends a slot the
    moment it has its frames (its natural end included), which the driver is told with `ended` after that step."""
    r = random.Random(1000 + seed)
    eng = (HoldFakeEngine if hold else TextFakeEngine)()
    eng.open(B)
    ev, want = ["open %d %d %d" % (B, hold, 64)], [None]

    def did(event, before, steps=0):
        rows, starved = eng.text_state()
        ev.append(event)
        want.append((steps, list(eng.frames), list(getattr(eng, "held", [0] * B)), [int(x) for x in starved], before))

    def push(b, n, final):
        before = list(eng.ended)
        n = min(n, 50 - len(eng.text[b]["rows"]))      # (the fake's reservation)
        eng.push_text(b, np.zeros((n, 1024), np.float32), bool(final), 0)
        did("push %d %d %d" % (b, n, final), before)

    for _ in range(60):
        free = [b for b in range(B) if eng.ended[b]]
        texts = [b for b in range(B) if not eng.ended[b] and eng.text[b] and not eng.text[b]["final"]]
        live = [b for b in range(B) if not eng.ended[b]]
        op = r.choice(["admit", "push", "run", "run", "run", "run", "run", "release"])
        before = list(eng.ended)
        if op == "admit" and free:
            b, budget, text = r.choice(free), r.randint(1, 12), r.randrange(2)
            sp = dataclasses.replace(DEFAULTS, max_frames=budget, text_stream=bool(text))
            eng.admit([b], [np.full((1, 1), 7, np.float32)], [budget], [sp])
            did("admit %d %d %d" % (b, budget, text), before)
            if text and r.random() < 0.8:              # a server admits a text slot with its first rows at hand
                push(b, r.randint(1, 3), 0)
        elif op == "push" and texts:
            push(r.choice(texts), r.randrange(4), int(r.random() < 0.25))
        elif op == "run":
            steps = eng.run(1)
            did("run 1", before, steps)
            for b in range(B):
                if eng.ended[b] and not before[b]:
                    ev.append("ended %d" % b)
                    want.append(None)
        elif op == "release" and live:
            b = r.choice(live)
            eng.release([b])
            did("release %d" % b, before)
    return ev, want


@pytest.mark.parametrize("hold", [0, 1])
def test_the_fake_engines_play_the_same_rules(driver, hold):
    n_runs = n_held = n_stalled = 0
    for seed in range(60):
        B = (1, 2, 5)[seed % 3]
        ev, want = replay_through_fake(driver, seed, B, hold)
        for line, e, w in zip(play(driver, ev), ev, want):
            if w is None:
                continue
            (room, steps), slots = cells(line)
            f_steps, frames, held, starved, was_ended = w
            if e.startswith("run"):
                assert steps == f_steps, (seed, e, line, w)
                n_runs += 1
                n_stalled += steps == 0
            for b in range(B):
                if was_ended[b]:
                    continue      # (the fake stops a slot's counters where it ends; the engine's rows step on, idle)
                assert slots[b][0] == frames[b] and slots[b][1] == held[b] and slots[b][2] == starved[b], (seed, e, b, line, w)
                n_held += held[b]
    assert n_runs > 500 and n_stalled > 50 and (n_held > 500 if hold else n_held == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the prefix cache's index (q3e_prefix_cache / q3e_admit_keyed / q3e_prefix_stats)


class IndexModel:
    def __init__(self):
        self.n = self.max_rows = self.clock = 0
        self.entries = {}          # entry -> (key, n_rows, last use)
        self.stats = dict(hits=0, misses=0, stores=0, evictions=0, too_long=0)

    def resize(self, n, max_rows):
        self.n, self.max_rows, self.entries = n, (max_rows if n else 0), {}      # drops every entry; the counters run on

    def key(self, k0, k1, n_rows):
        st = self.stats
        if (k0, k1) == (0, 0):
            return "unkeyed", -1
        if self.n and n_rows > self.max_rows:
            st["too_long"] += 1
            return "too_long", -1
        at = [i for i, (k, _, _) in self.entries.items() if k == (k0, k1)]
        self.clock += 1
        if at and self.entries[at[0]][1] == n_rows:
            st["hits"] += 1
            self.entries[at[0]] = ((k0, k1), n_rows, self.clock)
            return "hit", at[0]
        st["misses"] += 1
        if not self.n:
            return "no_pool", -1
        if at:                                            # present with another n_rows: a miss that replaces that entry
            i = at[0]
        elif len(self.entries) < self.n:                  # a free entry
            i = min(set(range(self.n)) - set(self.entries))
        else:                                             # the least recently used one (use = hit or store)
            i = min(self.entries, key=lambda j: self.entries[j][2])
            st["evictions"] += 1
        st["stores"] += 1
        self.entries[i] = ((k0, k1), n_rows, self.clock)
        return "miss", i

    def line(self, what, entry):
        st = self.stats
        return "pfx %s %d %d %d %d %d %d %d" % (what, entry, st["hits"], st["misses"], st["stores"], st["evictions"],
                                                st["too_long"], len(self.entries))


def expect_index(events):
    m, out = IndexModel(), []
    for ev in events:
        op, *a = ev.split()
        a = [int(x) for x in a]
        if op == "pfx":
            m.resize(*a)
            out.append(m.line("-", -1))
        else:
            out.append(m.line(*m.key(*a)))
    return out


INDEX = {
    "hit": ["pfx 2 32", "key 5 6 12", "key 5 6 12", "key 5 6 12"],
    "miss_into_a_free_entry": ["pfx 3 32", "key 1 0 8", "key 0 1 8", "key 1 1 9", "key 0 0 9"],
    "eviction_in_lru_order": ["pfx 3 32", "key 1 1 8", "key 2 2 8", "key 3 3 8", "key 1 1 8", "key 4 4 8", "key 2 2 8",
                              "key 5 5 8", "key 1 1 8", "key 3 3 8"],
    "same_key_another_length": ["pfx 2 32", "key 7 7 10", "key 8 8 10", "key 7 7 11", "key 7 7 10", "key 7 7 10", "key 8 8 10"],
    "too_long": ["pfx 2 16", "key 9 9 17", "key 9 9 16", "key 9 9 17", "key 9 9 16"],
    "pool_of_0_entries": ["key 3 4 8", "key 3 4 8", "pfx 0 0", "key 3 4 800", "key 0 0 8"],
    "resize": ["pfx 2 16", "key 1 2 8", "key 3 4 8", "pfx 4 32", "key 1 2 8", "key 1 2 8", "key 5 6 30", "pfx 0 0", "key 1 2 8"],
    "largest_keys": ["pfx 1 8", "key 18446744073709551615 0 4", "key 0 18446744073709551615 4", "key 0 18446744073709551615 4"],
}


@pytest.mark.parametrize("name", sorted(INDEX))
def test_prefix_index(driver, name):
    assert play(driver, INDEX[name]) == expect_index(INDEX[name])


def test_prefix_index_outcomes_named(driver):
    def classes(name):
        return [line.split()[1:3] for line in play(driver, INDEX[name])]
    assert classes("hit")[1:] == [["miss", "0"], ["hit", "0"], ["hit", "0"]]
    assert classes("eviction_in_lru_order")[5:] == [["miss", "1"], ["miss", "2"], ["miss", "0"], ["miss", "1"], ["miss", "2"]]
    assert classes("same_key_another_length")[3:5] == [["miss", "0"], ["miss", "0"]]      # the entry of the key, no victim
    assert play(driver, INDEX["same_key_another_length"])[-1] == "pfx hit 1 2 4 4 0 0 2"
    assert classes("too_long")[1:] == [["too_long", "-1"], ["miss", "0"], ["too_long", "-1"], ["hit", "0"]]
    assert [c[0] for c in classes("pool_of_0_entries")] == ["no_pool", "no_pool", "-", "no_pool", "unkeyed"]


def test_prefix_index_random(driver):
    r = random.Random(11)
    ev = []
    for _ in range(3000):
        if r.random() < 0.01:
            ev.append("pfx %d %d" % (r.choice([0, 1, 3, 4]), r.choice([8, 16])))
        else:
            ev.append("key %d %d %d" % (r.randrange(3), r.randrange(3), r.choice([4, 8, 12, 20])))
    got, want = play(driver, ev), expect_index(ev)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, ev[max(0, i - 10):i + 1], g, w)
