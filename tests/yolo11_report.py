"""TEST INFRASTRUCTURE: the distances the YOLO11 GPU tests measure, collected per process.  With ``PADEL_YOLO11_REPORT`` set to a
file name they are also written there as JSON after every case; profiles/yolo11_parity.json is the record of one such run of
tests/test_gpu_yolo11_ops.py and tests/test_gpu_yolo11.py in one process."""
import json
import os

REPORT = {}


def record(tag: str, values: dict) -> None:
    REPORT[tag] = values
    path = os.environ.get("PADEL_YOLO11_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, default=str)
