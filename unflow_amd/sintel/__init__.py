"""MPI Sintel evaluation input (mirror of src/e2eflow/sintel/input.py): .flo ground truth with invalid and occlusion masks."""
