"""What tests/test_cpu_ring_triple.py needs beyond tests/ring_joint_cases.py (the step list, its reference and b32 are imported from
there): the hand-back allowance of the three-base form."""

# multipliers e of the step list (ring_joint_cases.LISTED_E) on which a three-base step may hand back, each with the intermediate sum that
# collides: {e: (level, half, accumulator multiplier mod n, operand multiplier mod n)} -- the addition at that level and half meets an
# operand with the accumulator's own x because the two multipliers are equal or opposite mod n.  At most two.  The host emulation completes
# every listed multiplier, so the allowance is empty (tests/test_cpu_ring_triple.py checks it).
HANDBACK_ALLOWED = {}
