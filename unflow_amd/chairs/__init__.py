"""FlyingChairs input (mirror of src/e2eflow/chairs/input.py): the test pairs with their .flo ground truth, and the raw pairs."""
