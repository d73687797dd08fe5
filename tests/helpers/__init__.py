"""Helper modules and child-process scripts of the test suite."""
