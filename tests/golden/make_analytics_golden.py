"""Generates tests/golden/analytics_golden.json by importing the reference's ``analytics/data_analytics.py`` in THIS
container (the reference never travels: only the recorded results below are committed).

The module needs pandas and numpy alone, both installed here; it is loaded by path, so that the reference's ``analytics``
package (whose ``__init__`` imports cv2 and supervision) is not.  Scripted sequences of ``add_player_position`` / ``step`` are
run through the reference's ``DataAnalytics`` and what it answers is recorded: ``into_dict`` and ``len()``, or the type name of
the exception where it raises, and one ``into_dataframe(30)`` with its column order (NaN written as null).

    python tests/golden/make_analytics_golden.py        # needs /root/reference
"""
import contextlib, importlib.util, io, json, math, warnings
from pathlib import Path

REF = "/root/reference/analytics/data_analytics.py"


def position(i: int, pid: int) -> tuple:
    """A scripted player path in metres: binary fractions and thirds, so that the derived columns meet rounding."""
    return (float(pid) - 2.5 + 0.125 * i + (i * i) / 3.0, -7.0 + 1.75 * pid + 0.3 * i * (1 if pid % 2 else -1))


# name -> one list of (id, frame index the position is taken from) per frame, in the order the positions are added
SEQUENCES = {
    "all_four": [[(1, i), (2, i), (3, i), (4, i)] for i in range(4)],
    "missing_player": [[(1, 0), (2, 0), (3, 0), (4, 0)], [(1, 1), (3, 1), (4, 1)], [(2, 2), (4, 2)]],
    "empty_frame": [[(1, 0), (2, 0), (3, 0), (4, 0)], [], [(1, 2), (2, 2), (3, 2), (4, 2)]],
    "all_empty": [[], []],
    "one_foreign_id": [[(1, 0), (2, 0), (7, 0), (3, 0), (4, 0)], [(1, 1), (2, 1), (3, 1), (4, 1), (19, 1)]],
    "unsorted_ids": [[(3, 0), (1, 0), (4, 0), (2, 0)], [(4, 1), (3, 1), (2, 1), (1, 1)]],
    "duplicate_id": [[(1, 0), (2, 0), (3, 0), (4, 0)], [(1, 1), (2, 1), (2, 1), (4, 1)]],
}
# the dataframe: 8 frames, player 3 missing in frame 2, nobody in frame 5, player 1 missing in frames 6 and 7
DATAFRAME = [[(p, i) for p in (1, 2, 3, 4) if not ((i == 2 and p == 3) or i == 5 or (i >= 6 and p == 1))] for i in range(8)]
FPS = 30


def run(mod, frames):
    da = mod.DataAnalytics()
    for adds in frames:
        for pid, i in adds:
            da.add_player_position(id=pid, position=position(i, pid))
        da.step(1)
    da.frames = da.frames[:-1]                    # the runner drops the extra frame after the clip
    return da


def main():
    spec = importlib.util.spec_from_file_location("reference_data_analytics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"fps": FPS, "sequences": {}}
    quiet = io.StringIO()
    warnings.simplefilter("ignore")              # (pandas: the reference adds its 169 columns one by one)
    for name, frames in SEQUENCES.items():
        entry = {"adds": [[[pid, list(position(i, pid))] for pid, i in adds] for adds in frames]}
        try:
            with contextlib.redirect_stdout(quiet):
                da = run(mod, frames)
                entry["into_dict"] = da.into_dict()
            entry["len"] = len(da)
        except Exception as exc:
            entry["raises"] = type(exc).__name__
        out["sequences"][name] = entry
    with contextlib.redirect_stdout(quiet):
        da = run(mod, DATAFRAME)
        df = da.into_dataframe(FPS)
    out["dataframe"] = {
        "adds": [[[pid, list(position(i, pid))] for pid, i in adds] for adds in DATAFRAME],
        "columns": list(df.columns),
        "values": {c: [None if (v is None or (isinstance(v, float) and math.isnan(v))) else (int(v) if c == "frame" else float(v))
                       for v in df[c].tolist()] for c in df.columns},
    }
    Path(__file__).with_name("analytics_golden.json").write_text(json.dumps(out, indent=1))
    print("wrote", len(out["sequences"]), "sequences and a dataframe of", len(df), "rows x", len(df.columns), "columns")


if __name__ == "__main__":
    main()
