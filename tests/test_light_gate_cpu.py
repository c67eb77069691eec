"""The launch gate of the three shadow-ray shortcuts (csrc/light_gate.h), no GPU: host/light_gate_check.cpp prints the gate's
decision for every combination of its inputs, and each line is held against the rules as include/svo.h states them ("Light clearance":
automatic / dropped by / used by / svo_world_prepared_bricks / dark at birth, and svo_trace_params.shadow) - written down here from that
text, not from the header under test."""
import itertools
import subprocess

from test_host_units import compile_host

NO_CLEARANCE, NO_BRICK_CLEARANCE, NO_DARK_BIRTH = 2, 4, 8       # bits of svo_trace_params.shadow
NODES, BRICKS, DARK = 1, 2, 4                                   # what a launch may use
STATES = ["FRESH", "DROPPED", "UNUSED", "NODES", "BRICKS"]


def rules(eligible, shadow, state, auto_work, same_dir, eps_pow2, eps_covers, dark_premises):
    """(what the launch uses, whether it prepares the world first).  `eligible`: "camera launches of SVO_SEMANTICS_CPU with shadow rays"
    on the stack kernel, none of what "march[es] every step as before"."""
    # "the first ... launch with shadow rays on a world that has not changed since its upload ... prepares the bits for its own light_dir",
    # "only while wide entries x chunks <= 1e10"; SVO_SHADOW_NO_CLEARANCE launches "march every step as before"
    prepare = eligible and state == "FRESH" and auto_work and not shadow & NO_CLEARANCE
    use = 0
    if eligible:
        # "whose light_dir equals the prepared one bit for bit and whose eps is a power of two of at least twice the float spacing";
        # "a direction with a non-zero component below 1/64 ... is accepted and never used" (UNUSED); dropped bits are not there
        bits = state in ("NODES", "BRICKS") and same_dir and eps_pow2 and eps_covers and not shadow & NO_CLEARANCE
        if bits:
            use |= NODES
        # "same lifecycle and the same launches as the bits; in addition the world must ..." (BRICKS); "SVO_SHADOW_NO_BRICK_CLEARANCE
        # switches the flags off alone, SVO_SHADOW_NO_CLEARANCE both"
        if bits and state == "BRICKS" and not shadow & NO_BRICK_CLEARANCE:
            use |= BRICKS
        # "needs none of the above ... no prepared light, no bit of the pools ... the same launches as the bits ... by default it is also
        # left off where eps is below twice the float spacing ... SVO_SHADOW_NO_DARK_BIRTH switches it off alone,
        # SVO_SHADOW_NO_BRICK_CLEARANCE with the flags, SVO_SHADOW_NO_CLEARANCE with everything"
        if dark_premises and eps_covers and not shadow & (NO_CLEARANCE | NO_BRICK_CLEARANCE | NO_DARK_BIRTH):
            use |= DARK
    return use, int(prepare)


def test_every_combination_of_the_gate_follows_the_header():
    exe = compile_host("light_gate_check.cpp", extra=["-I../csrc"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    seen = set()
    for line in r.stdout.splitlines():
        left, right = line.split(" -> ")
        e, shadow, state, *flags = left.split()
        key = (int(e), int(shadow), state, *map(int, flags))
        assert shadow_is_on(key[1]) and state in STATES
        assert tuple(map(int, right.split())) == rules(*key), line
        seen.add(key)
    want = set(itertools.product((0, 1), [1 | s for s in range(0, 16, 2)], STATES, *[(0, 1)] * 5))
    assert seen == want and len(want) == 2 * 8 * 5 * 32


def shadow_is_on(shadow):
    return shadow & 1 == 1


def test_the_rules_themselves():
    """A few lines by hand, so that a slip in `rules` does not pass with the same slip in the header."""
    on = (1, 1, 1, 1, 1)                                                    # auto_work, same_dir, eps_pow2, eps_covers, dark_premises
    assert rules(1, 1, "BRICKS", *on) == (NODES | BRICKS | DARK, 0)
    assert rules(1, 1, "NODES", *on) == (NODES | DARK, 0)
    assert rules(1, 1, "UNUSED", *on) == (DARK, 0)                          # prepared and unused: no launch prepares it again
    assert rules(1, 1, "DROPPED", *on) == (DARK, 0)                         # after an edit dark at birth still holds
    assert rules(1, 1, "FRESH", *on) == (DARK, 1)
    assert rules(1, 1, "FRESH", 0, 1, 1, 1, 1) == (DARK, 0)                 # too large to prepare on its own
    assert rules(1, 1 | NO_CLEARANCE, "FRESH", *on) == (0, 0)
    assert rules(1, 1 | NO_BRICK_CLEARANCE, "BRICKS", *on) == (NODES, 0)
    assert rules(1, 1 | NO_BRICK_CLEARANCE, "FRESH", *on) == (0, 1)
    assert rules(1, 1 | NO_DARK_BIRTH, "BRICKS", *on) == (NODES | BRICKS, 0)
    assert rules(1, 1, "BRICKS", 1, 0, 1, 1, 1) == (DARK, 0)                # another light than the prepared one
    assert rules(1, 1, "BRICKS", 1, 1, 0, 1, 1) == (DARK, 0)                # dark at birth: any eps that covers the spacing
    assert rules(1, 1, "BRICKS", 1, 1, 1, 0, 1) == (0, 0)
    assert rules(0, 1, "BRICKS", *on) == (0, 0) and rules(0, 1, "FRESH", *on) == (0, 0)
