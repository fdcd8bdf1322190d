"""The importable part of the reference's aerial_gym/examples: code its example scripts import from each other.  The runnable
scripts live in examples/ at the repository root."""
