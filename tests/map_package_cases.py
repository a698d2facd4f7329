"""The plans the map package's host half is checked on, shared by the C ABI test (test_map_package_capi.py) and the C++ one
(test_map_package_cpp.py), both against tests/map_package_ref.py.  Coordinates are small integers or binary fractions wherever a case
is about a comparison that must come out exactly."""
import numpy as np


def plan_cases():
    """{name: (translations [n, 3], border_offset, piece_width)} -- every one of them is accepted."""
    line = np.array([[10.0 * k, 5.0, 0.0] for k in range(5)])
    rng = np.random.default_rng(11)
    return {
        # one submap, the reference's defaults: one piece that holds the whole map
        "one_submap": (np.array([[3.0, 4.0, 1.0]]), 100.0, 500.0),
        # a straight line and no border: the y extent is 0, y_steps 0 becomes 1; the x extent 40 is exactly 5 half widths
        "line_exact_multiple": (line, 0.0, 16.0),
        # ... and just short of it: 4 steps (truncation)
        "line_just_short": (np.array([[0.0, 5.0, 0.0], [39.999999, 5.0, 0.0]]), 0.0, 16.0),
        # submaps at x = 0 and x = 12 lie exactly on the widened bounds [0, 12] of piece 1 (box [2, 10], border 2): closed tests keep both
        "on_the_widened_bound": (np.array([[0.0, 0.0, 0.0], [12.0, 0.0, 0.0], [20.0, 0.0, 0.0]]), 2.0, 8.0),
        # the last pieces' boxes reach beyond the extent and are clamped to it
        "clamped_outer_pieces": (np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 1.0, 0.0], [21.0, 13.0, 0.0]]), 2.0, 8.0),
        # a negative border that inverts the extent by less than half a piece: the step count truncates to 0, becomes 1, and is NOT refused
        "slightly_inverted": (np.array([[1.0, 1.0, 0.0]]), -1.0, 8.0),
        # a two-dimensional walk with irrational coordinates
        "walk": (np.cumsum(rng.normal(0, 7, (40, 3)), axis=0), 3.7, 21.3),
    }


def refused_cases():
    """{name: (translations, border_offset, piece_width, the reference refuses it too)}"""
    two = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    return {
        "inverted_extent": (two, -30.0, 8.0, True),                   # (10 + 2 * -30) / 4 = -12 steps
        "piece_width_zero": (two, 2.0, 0.0, False),
        "piece_width_negative": (two, 2.0, -8.0, False),
        "piece_width_nan": (two, 2.0, float("nan"), False),
        "piece_width_inf": (two, 2.0, float("inf"), False),
        "border_nan": (two, float("nan"), 8.0, False),
        "border_inf": (two, float("inf"), 8.0, False),
        "too_many_pieces": (np.array([[0.0, 0.0, 0.0], [1000.0, 1000.0, 0.0]]), 0.0, 2.0, False),   # 1000 x 1000
        "one_row_too_many": (np.array([[0.0, 0.0, 0.0], [65537.0, 0.0, 0.0]]), 0.0, 2.0, False),   # 65537 x 1
        "no_submap": (np.zeros((0, 3)), 2.0, 8.0, False),
        "translation_nan": (np.array([[0.0, float("nan"), 0.0]]), 2.0, 8.0, False),
    }
