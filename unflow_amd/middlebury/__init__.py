"""Middlebury evaluation input (mirror of src/e2eflow/middlebury/input.py) and the .flo readers the other datasets share."""
