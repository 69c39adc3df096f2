"""MI355X-native batch-SOM engine behind the XPySom class surface of jcfaracco/xpysom-dask."""
from .xpysom import EpochRecord, UnitMeans, UnitStatistics, XPySom

__all__ = ["XPySom", "UnitStatistics", "UnitMeans", "EpochRecord"]
