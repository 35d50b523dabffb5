from .attribute_user_knn import AttributeUserKNN  # noqa: F401
