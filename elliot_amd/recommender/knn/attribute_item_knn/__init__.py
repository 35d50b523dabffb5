from .attribute_item_knn import AttributeItemKNN  # noqa: F401
