from .analytics import DataAnalytics, DataPoint, InvalidDataPoint, PlayerPosition  # noqa: F401
