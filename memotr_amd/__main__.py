"""``python -m memotr_amd``: see main.py."""
from .main import main

if __name__ == "__main__":
    main()
