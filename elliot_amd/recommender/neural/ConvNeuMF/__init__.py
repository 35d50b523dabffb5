from .convolutional_neural_matrix_factorization import ConvNeuMF  # noqa: F401
